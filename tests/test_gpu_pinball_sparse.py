"""solver.pinball and the MatrixConstraintBase operations on a constraint matrix kept sparse
(matrix.sparse(method="constraint")), against the numpy restatement of tests/pinball_checks.py on the same array (structural
zeros are exact zeros to it) and against the dense route on A.toarray().  The bounds are those of test_gpu_pinball.py, imported:
they hold a fortiori with fewer terms per dot.  test_pinball_sparse_host.py shows that every case qualifies for the exact
checks.  Every test prints the figures it asserts on."""
import os
import re
import sys
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import adelie_amd as ad
from adelie_amd import _abi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pinball_checks as pc  # noqa: E402
import pinball_sparse_checks as ps  # noqa: E402
from test_gpu_pinball import (EPS32, EPS64, check_close, check_exact, check_invariants, err, same_state, set_config,  # noqa: E402
                              sets_of)

pytestmark = pytest.mark.gpu

CASES = [g + (s,) for g in ps.GRID for s in ps.SEEDS]
# more than one wavefront of members | H appended 7 at a time | rows of more than a wavefront and a tile
BOTH_ROUTES = [ps.GRID[2], ps.GRID[4], ps.GRID[6]]


def sparse_of(A):
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # a csr_matrix is taken as it is
        return ad.matrix.sparse(sp.csr_matrix(np.array(A)), method="constraint")


def run(inputs, **kw):
    A, S, v, pneg, ppos = inputs
    return ad.pinball(sparse_of(A), S, v, pneg, ppos, **kw)


def run_dense(inputs, **kw):
    A, S, v, pneg, ppos = inputs
    return ad.pinball(ad.matrix.dense(np.array(A), method="constraint"), S, v, pneg, ppos, **kw)


@pytest.mark.parametrize("m, d", [(37, 1), (5, 70), (300, 33)])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_constraint_matrix_operations(hip, m, d, dtype):
    """Against numpy in float64; the bound is k eps sum |a| |b| per dot of k terms (nested dots add their terms), as in
    test_gpu_pinball.py::test_constraint_matrix_operations."""
    rs = np.random.RandomState(m + d)
    A = (rs.normal(size=(m, d)) * (rs.uniform(size=(m, d)) < 0.2)).astype(dtype)
    A[m // 2 - 1] = 0  # an empty row
    if d > 1:
        A[m // 2, :2] = 1.5  # (the row the row operations use is not empty)
    else:
        A[m // 2] = 1.5
    eps = float(np.finfo(dtype).eps)
    A64, aA = A.astype(np.float64), np.abs(A.astype(np.float64))
    for form in (sp.csr_matrix, sp.csc_matrix):
        mat = form(A)
        if form is sp.csc_matrix:
            with pytest.warns(UserWarning, match="Converting to CSR format."):
                M = ad.matrix.sparse(mat, method="constraint")
        else:
            with warnings.catch_warnings():
                warnings.simplefilter("error")
                M = ad.matrix.sparse(mat, method="constraint")
        assert isinstance(M, ad.matrix.MatrixConstraintBase64 if dtype == np.float64 else ad.matrix.MatrixConstraintBase32)
        assert (M.rows(), M.cols(), M.shape, M.ndim, M.dtype) == (m, d, (m, d), 2, dtype)
        dense = M.to_dense()
        assert dense.dtype == dtype and dense.flags.c_contiguous and np.array_equal(dense, mat.toarray())
        worst = 0.0

        def close(got, want, bound, what):
            nonlocal worst
            e = np.abs(np.asarray(got, dtype=np.float64) - want)
            worst = max(worst, float(np.max(e / np.maximum(bound, np.finfo(np.float64).tiny))))
            assert np.all(e <= bound), what

        v = rs.normal(size=d).astype(dtype)
        w = rs.normal(size=m).astype(dtype)
        Q = rs.normal(size=(d, d)).astype(dtype)
        v64, w64, Q64 = v.astype(np.float64), w.astype(np.float64), Q.astype(np.float64)
        out = np.empty(m, dtype=dtype)
        M.tmul(v, out)
        close(out, A64 @ v64, (d + 1) * eps * (aA @ np.abs(v64)), "tmul")
        out = np.empty(d, dtype=dtype)
        M.mul(w, out)
        close(out, w64 @ A64, (m + 1) * eps * (np.abs(w64) @ aA), "mul")
        idx = rs.choice(m, size=min(m, 4), replace=False)
        idx = np.concatenate([idx, idx[:2], idx[:1]])  # repeated indices: their values add up
        val = rs.normal(size=idx.size).astype(dtype)
        val64 = val.astype(np.float64)
        M.sp_mul(idx, val, out)
        close(out, val64 @ A64[idx], (idx.size + 1) * eps * (np.abs(val64) @ aA[idx]), "sp_mul")
        j = m // 2
        M.rmmul(j, Q, out)
        close(out, A64[j] @ Q64, (d + 1) * eps * (aA[j] @ np.abs(Q64)), "rmmul")
        M.rmmul_safe(j, Q, out)
        close(out, A64[j] @ Q64, (d + 1) * eps * (aA[j] @ np.abs(Q64)), "rmmul_safe")
        for f in (M.rvmul, M.rvmul_safe):
            close(f(j, v), A64[j] @ v64, (d + 1) * eps * (aA[j] @ np.abs(v64)), "rvmul")
            assert f(j - 1, v) == 0  # the empty row
        start = rs.normal(size=d).astype(dtype)
        out = start.copy()
        M.rvtmul(j, dtype(0.75), out)
        close(out, start.astype(np.float64) + 0.75 * A64[j], 2 * eps * (np.abs(start.astype(np.float64)) + 0.75 * aA[j]), "rvtmul")
        C = np.empty((m, m), dtype=dtype)
        M.cov(Q, C)  # (Q is not symmetric: a transposed product would miss)
        close(C, A64 @ Q64 @ A64.T, (2 * d + 2) * eps * (aA @ np.abs(Q64) @ aA.T), "cov")
        print(f"({m}, {d}) {np.dtype(dtype).name} {form.__name__}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("m, d, kappa, pen, density, wide, seed", CASES)
def test_float64_grid(hip, m, d, kappa, pen, density, wide, seed):
    inputs = ps.cached_inputs(m, d, seed, pen, density, wide)
    own = ps.cached_run(m, d, seed, pen, density, wide, kappa, "float64")
    print(f"restatement: ns {len(own.screen)}, active {len(own.active)}, iters {own.iters}, n_kkt {own.n_kkt}, exit {own.exit}, "
          f"min_gap {own.min_gap:.3e}")
    assert own.min_gap >= ps.GAP64  # every grid case qualifies: nothing is skipped
    state = run(inputs, kappa=kappa)
    assert state.error == own.error == ""
    assert state.beta.dtype == np.float64 and state.beta.shape == (m,) and state.resid.shape == (d,)
    check_exact(state, own)
    truth = ps.cached_run(m, d, seed, pen, density, wide, kappa, "longdouble")
    assert truth.screen == own.screen and truth.active == own.active and truth.iters == own.iters
    check_close(state, own, truth, inputs, EPS64)
    check_invariants(state, inputs)
    print(f"changed visits: device {state.benchmark['n_changed']:.0f}, restatement {own.n_changed}")


@pytest.mark.parametrize("m, d, kappa, pen, density, wide", ps.GRID32)
@pytest.mark.parametrize("seed", ps.SEEDS)
def test_float32_grid(hip, m, d, kappa, pen, density, wide, seed):
    inputs = ps.cached_inputs(m, d, seed, pen, density, wide, True)  # A, S, v rounded to float32
    truth = ps.cached_run(m, d, seed, pen, density, wide, kappa, "float64", True)
    own = ps.cached_run(m, d, seed, pen, density, wide, kappa, "float32", True)
    state = run(inputs, kappa=kappa)
    assert state.error == ""
    assert state.beta.dtype == np.float32 and state.resid.dtype == np.float32 and state.screen_AS.dtype == np.float32
    print(f"float64 restatement on the rounded inputs: min_gap {truth.min_gap:.3e}")
    if truth.min_gap >= ps.GAP32:
        assert own.screen == truth.screen and own.active == truth.active
        check_exact(state, truth)
    check_close(state, own, truth, inputs, EPS32)
    check_invariants(state, inputs)
    same_state(state, run(inputs, kappa=kappa))


@pytest.mark.parametrize("m, d, kappa, pen, density, wide", BOTH_ROUTES)
def test_sparse_and_dense_routes_agree(hip, m, d, kappa, pen, density, wide):
    """The two routes on the same matrix: the same trajectory, the same numbers in A_S S and diag(A_S S A_S') (every skipped
    term is an exact no-op), and beta / resid each within check_close's bound of the truth."""
    inputs = ps.cached_inputs(m, d, 0, pen, density, wide)
    own = ps.cached_run(m, d, 0, pen, density, wide, kappa, "float64")
    truth = ps.cached_run(m, d, 0, pen, density, wide, kappa, "longdouble")
    sparse, dense = run(inputs, kappa=kappa), run_dense(inputs, kappa=kappa)
    assert sparse.error == dense.error == ""
    assert sets_of(sparse) == sets_of(dense)
    assert (sparse.iters, sparse.n_kkt) == (dense.iters, dense.n_kkt)
    assert np.array_equal(sparse.screen_AS, dense.screen_AS)
    assert np.array_equal(sparse.screen_ASAT_diag, dense.screen_ASAT_diag)
    print(f"ns {sparse.screen_set_size}, iters {sparse.iters}, n_kkt {sparse.n_kkt}; sparse vs dense: beta "
          f"{err(sparse.beta, dense.beta):.3e}, resid {err(sparse.resid, dense.resid):.3e}")
    check_close(sparse, own, truth, inputs, EPS64, "sparse ")
    check_close(dense, own, truth, inputs, EPS64, "dense ")


def test_global_storage_gives_the_same_bits(hip):
    m, d, kappa, pen, density, wide = ps.GRID[2]
    inputs = ps.cached_inputs(m, d, 0, pen, density, wide)
    in_lds = run(inputs)
    try:
        set_config("pinball_lds_max_ns", 1)
        in_global = run(inputs)
    finally:
        set_config("pinball_lds_max_ns", 0)
    assert in_lds.screen_set_size > 1
    same_state(in_lds, in_global)
    check_exact(in_global, ps.cached_run(m, d, 0, pen, density, wide, kappa, "float64"))


def test_rerun_gives_the_same_bits(hip):
    m, d, kappa, pen, density, wide = ps.GRID[4]
    inputs = ps.cached_inputs(m, d, 0, pen, density, wide)
    same_state(run(inputs, kappa=kappa), run(inputs, kappa=kappa))


def test_gram_limit(hip):
    m, d, kappa, pen, density, wide = ps.GRID[2]
    inputs = ps.cached_inputs(m, d, 0, pen, density, wide)
    try:
        set_config("pinball_gram_limit_mb", 0.001)
        state = run(inputs)
    finally:
        set_config("pinball_gram_limit_mb", 16384)
    found = re.fullmatch(r"adelie_core solver: pinball: screen set of (\d+) coordinates exceeds the device Gram limit", state.error)
    assert found, state.error
    assert int(found.group(1)) ** 2 * 8 > 0.001 * (1 << 20)
    check_invariants(state, inputs)
    assert run(inputs).error == ""


def test_warm_start(hip):
    """extend(0, ns) and the sweep of the listed rows."""
    m, d, kappa, pen, density, wide = ps.GRID[2]
    inputs = ps.cached_inputs(m, d, 0, pen, density, wide)
    A, S, v, pneg, ppos = inputs
    coarse = run(inputs, tol=1e-4)
    own1 = ps.cached_run(m, d, 0, pen, density, wide, kappa, "float64", tol=1e-4)
    truth1 = ps.cached_run(m, d, 0, pen, density, wide, kappa, "longdouble", tol=1e-4)
    assert own1.min_gap >= ps.GAP64
    check_exact(coarse, own1)
    fine = run(inputs, tol=1e-9, warm_start=coarse)
    own2 = pc.solve(A, S, v, pneg, ppos, np.float64, tol=1e-9, warm_start=own1)
    truth2 = pc.solve(A, S, v, pneg, ppos, np.longdouble, tol=1e-9, warm_start=truth1)
    print(f"warm restatement: ns {len(own2.screen)}, iters {own2.iters}, n_kkt {own2.n_kkt}, min_gap {own2.min_gap:.3e}")
    assert fine.error == "" and own2.min_gap >= ps.GAP64
    check_exact(fine, own2)
    check_close(fine, own2, truth2, inputs, EPS64)
    check_invariants(fine, inputs)
    again = run(inputs, tol=1e-9, warm_start=fine)
    assert again.error == "" and again.screen_set_size == fine.active_set_size  # no admissions from the solution
    assert sets_of(again)[0] == sets_of(fine)[1]


@pytest.mark.parametrize("seed", ps.SEEDS)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_edge_inputs(hip, dtype, seed):
    """Infinite penalties on either side (inf itself in float32), a zero row (v_k = 0, no stored entry) and a repeated row."""
    r32 = dtype == "float32"
    key = ("edge", 0, seed, 1.0, ps.EDGE_DENSITY, False)
    inputs = ps.cached_inputs(*key, r32)
    own = ps.cached_run(*key, None, dtype, r32)
    truth = ps.cached_run(*key, None, "float64" if r32 else "longdouble", r32)
    print(f"restatement: ns {len(own.screen)}, min_gap {own.min_gap:.3e}; wider format: min_gap {truth.min_gap:.3e}")
    state = run(inputs)
    assert state.error == ""
    if not r32:
        assert own.min_gap >= ps.GAP64
        check_exact(state, own)
    elif truth.min_gap >= ps.GAP32:
        check_exact(state, truth)
    check_close(state, own, truth, inputs, EPS32 if r32 else EPS64)
    check_invariants(state, inputs)
    assert np.all(state.beta[::2] >= 0) and np.all(state.beta[1::4] <= 0)
    assert state.beta[5] == 0  # the zero row is never changed
    if r32:
        assert np.isinf(state.penalty_neg[0]) and np.isinf(state.penalty_pos[1])


def test_naive_entry_points_refuse_the_sparse_constraint_matrix(hip):
    A, S, v, pneg, ppos = ps.cached_inputs(20, 5, 0, 1.0, 0.4)
    M = sparse_of(A)
    with pytest.raises(RuntimeError, match="constraint matrix"):
        ad.bvls(M, np.zeros(5), np.zeros(20), np.ones(20))
    with pytest.raises(RuntimeError, match="constraint matrix"):
        ad.grpnet(M, ad.glm.gaussian(np.zeros(5)))
    with pytest.raises(RuntimeError, match="not a constraint matrix"):
        ad.matrix.standardize(M)
    with pytest.raises(RuntimeError, match="not a constraint matrix"):
        ad.matrix.subset(M, np.arange(3), axis=1)
    with pytest.raises(RuntimeError, match="not a constraint matrix"):
        ad.matrix.concatenate([M, M], axis=0)
    # the core refuses the handle itself, in the words it has for the dense constraint handle
    b = M._backend
    out = np.zeros(20)
    ones = np.ones(5)
    assert b.fn("design_mul")(M._handle, ones.ctypes.data, ones.ctypes.data, out.ctypes.data) != 0
    assert "not a constraint matrix" in b.fn("last_error")().decode()
    handle = _abi.C.c_void_p()
    assert b.fn("design_alias")(M._handle, handle) != 0
    assert "not a constraint matrix" in b.fn("last_error")().decode()
    cen, sc = np.zeros(20), np.ones(20)
    assert b.fn("design_create_standardized")(M._handle, cen.ctypes.data, sc.ctypes.data, handle) != 0
    assert "not a constraint matrix" in b.fn("last_error")().decode()
    srcs = (_abi.C.c_void_p * 2)(M._handle, M._handle)
    assert b.fn("design_create_concat")(srcs, 2, 1, handle) != 0
    assert "not a constraint matrix" in b.fn("last_error")().decode()
    rows = np.arange(3, dtype=np.int64)
    assert b.fn("design_create_derived")(M._handle, rows.ctypes.data, 3, None, 0, None, None, handle) != 0
    assert "not a constraint matrix" in b.fn("last_error")().decode()
    bargs = _abi.BvlsArgs()
    assert b.fn("bvls_solve")(M._handle, _abi.C.byref(bargs), handle) != 0
    assert "plain dense design" in b.fn("last_error")().decode()
    with pytest.raises(ValueError, match="'naive' or 'cov'"):
        ad.matrix.sparse(sp.csr_matrix(np.array(A)), method="lazy")


def test_constraint_linear_reads_the_kept_matrix(hip):
    rs = np.random.RandomState(5)
    m, d = 6, 4
    A = rs.normal(size=(m, d)) * (rs.uniform(size=(m, d)) < 0.5)
    A[0, 0] = 1.0
    mat = sp.csr_matrix(A)
    M = ad.matrix.sparse(mat, method="constraint")
    lower, upper = -rs.uniform(0.1, 1, m), rs.uniform(0.1, 1, m)
    from adelie_amd import constraint as cons
    host = cons._constraint_matrix_to_host(M)
    assert sp.issparse(host) and np.array_equal(host.toarray(), A)
    quad, lin = rs.uniform(1, 2, d), 3 * rs.normal(size=d)
    Q = np.linalg.qr(rs.normal(size=(d, d)))[0]
    results = []
    for mat_in in (M, mat):
        c = ad.constraint.linear(mat_in, lower, upper)
        assert c.primals() == d and c.duals() == m
        x = np.zeros(d)
        c.solve(x, quad, lin, 0.1, 0.05, Q)
        results.append((x.copy(), np.array(c._mu, dtype=float)))
    print("x:", results[0][0], "mu:", results[0][1])
    assert np.any(results[0][1] != 0)  # (some constraint binds: the solve did read the matrix)
    assert np.array_equal(results[0][0], results[1][0])
    assert np.array_equal(results[0][1], results[1][1])
