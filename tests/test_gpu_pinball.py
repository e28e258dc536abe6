"""solver.pinball on the device against the numpy restatement of tests/pinball_checks.py (itself checked against scipy and a
KKT certificate in test_pinball_host.py).  Wherever no decision of the restatement hangs on rounding (its min_gap is far above
the rounding of the format) the device must reproduce the whole trajectory: the ordered screen and active sets, the flags,
iters and n_kkt.  beta, resid and loss must be as close to a run of the restatement in the next wider format as a correct
implementation in the format can be expected to be: within 8x the restatement's own error (the margin of test_gpu_bvls.py) plus
an additive rounding term (check_close).  Every test prints the figures it asserts on."""
import os
import re
import sys

import numpy as np
import pytest

import adelie_amd as ad
from adelie_amd import _abi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pinball_checks as pc  # noqa: E402

pytestmark = pytest.mark.gpu

# (m, d, kappa, pen, max_iters): d = 1 | small | m = d | more than one wavefront | m < d: H of rank m | 17-20 KKT rounds, H
# appended 7 at a time | the larger ns | more than one trip of a 1024-thread workgroup, ends by the max-iterations exit
GRID = [(3, 1, None, 1.0, None), (20, 5, None, 1.0, None), (10, 10, None, 1.0, None), (130, 40, None, 0.3, None),
        (40, 100, None, 0.3, None), (300, 64, 7, 0.1, None), (2000, 100, None, 0.1, None)]
BIG = (1300, 200, 1300, 0.002, 25)
CASES = [g + (s,) for g in GRID for s in range(3)] + [BIG + (s,) for s in range(2)]
GRID32 = [(3, 1, None, 1.0), (10, 10, None, 1.0), (40, 100, None, 0.3)]
GAP64 = 1e-9
GAP32 = 1e-3
EPS64, EPS32 = np.finfo(np.float64).eps, np.finfo(np.float32).eps
MAX_ITERS = int(1e5)


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


def check_close(state, own, truth, inputs, eps, what=""):
    """device vs truth within 8x (own vs truth) + an additive rounding term; returns the largest device / bound ratio.

    The additive term is what the device's arithmetic adds to the restatement's.  The restatement recomputes g_k = A[k] . resid
    at every visit; the device updates g_a -= H[a, k] del at every changed visit: one rounding per element of a column of H (ns
    elements feed one coordinate's gradient over a pass), and H[a, k] = A[a] . AS[k] is a d-term dot of entries AS[k, j] that
    are d-term dots themselves: 2 d roundings.  So (ns + 2 d) eps times the scale of the quantity: max(1, max|beta|) for beta,
    max(|v| + |S| |A'| |beta|) (the terms of v - S A' beta) for resid.  The loss moves by one rounded update per pass and
    coordinate at most; its own scale is y_var / 2, so iters eps y_var as in test_gpu_bvls.py."""
    A, S, v = (np.asarray(x, dtype=np.float64) for x in inputs[:3])
    ns = max(len(truth.screen), 1)
    d = A.shape[1]
    y_var = float(truth.y_var)
    b = np.abs(np.asarray(truth.beta, dtype=np.float64))
    r_scale = float(np.max(np.abs(v) + np.abs(S) @ (np.abs(A).T @ b)))
    k = ns + 2 * d
    rows = [
        ("beta", err(state.beta, truth.beta), err(own.beta, truth.beta), k * eps * max(1.0, float(np.max(b)))),
        ("resid", err(state.resid, truth.resid), err(own.resid, truth.resid), k * eps * r_scale),
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


def check_invariants(state, inputs):
    """resid, loss, screen_ASAT_diag and screen_AS of the returned state, recomputed in float64 from the state's beta.

    resid starts as v (exact) or, on a warm start, as a rounded v - S A' beta (2 d + m terms); each fit catches it up by a dot
    of at most ns + 1 terms per entry whose AS entries are d-term dots: ((n_kkt + 1) (ns + 2) + 2 d + m_warm) eps times the
    scale max(|v| + |S| |A'| |beta|).  The loss moves by one rounded update per changed visit, at most iters * ns of them, each
    of scale y_var; recomputing it from the state's rounded resid moves it by |S^{-1} r| . (resid bound).  AS[k, j] is a d-term
    dot, v_k = A[k] . AS[k] a d-term dot of those: (d + 1) eps (|A_k| |S|)_j and (2 d + 2) eps |A_k| |S| |A_k|'."""
    A, S, v, pneg, ppos = inputs
    dtype = state.beta.dtype
    eps = float(np.finfo(dtype).eps)
    A64, S64, v64, b64 = (np.asarray(x, dtype=np.float64) for x in (A, S, v, state.beta))
    m, d = A64.shape
    ns = state.screen_set_size
    scale = float(np.max(np.abs(v64) + np.abs(S64) @ (np.abs(A64).T @ np.abs(b64))))
    r_err = err(state.resid, v64 - S64 @ (A64.T @ b64))
    r_bound = ((state.n_kkt + 1) * (ns + 2) + 2 * d + m) * eps * scale
    r64 = state.resid.astype(np.float64)
    sol = np.linalg.solve(S64, r64)
    y_var = float(v64 @ np.linalg.solve(S64, v64))
    l_err = abs(state.loss - 0.5 * float(r64 @ sol))
    l_bound = max(state.iters * max(ns, 1), 1) * eps * y_var + float(np.sum(np.abs(sol))) * r_bound
    print(f"resid vs v - S A' beta: {r_err:.3e} (bound {r_bound:.3e}); loss vs 1/2 r' S^-1 r: {l_err:.3e} (bound {l_bound:.3e})")
    assert r_err <= r_bound
    assert l_err <= l_bound
    mem = state.screen_set[:ns]
    assert state.screen_AS.shape == (m, d) and state.screen_ASAT_diag.shape == (m,)
    if ns:
        absAS = np.abs(A64[mem]) @ np.abs(S64)
        as_miss = np.abs(state.screen_AS[mem].astype(np.float64) - A64[mem] @ S64) - (d + 1) * eps * absAS
        dg = np.einsum("ij,ij->i", A64[mem] @ S64, A64[mem])
        dg_miss = np.abs(state.screen_ASAT_diag[mem].astype(np.float64) - np.maximum(dg, 0)) \
            - (2 * d + 2) * eps * np.einsum("ij,ij->i", absAS, np.abs(A64[mem]))
        print(f"screen_AS miss over bound: {float(np.max(as_miss)):.3e}; screen_ASAT_diag: {float(np.max(dg_miss)):.3e} (<= 0 passes)")
        assert np.all(as_miss <= 0) and np.all(dg_miss <= 0)
    with np.errstate(over="ignore"):
        inf_neg = ~np.isfinite(np.minimum(pneg, pc.MAX_SOLVER_VALUE).astype(dtype))
        inf_pos = ~np.isfinite(np.minimum(ppos, pc.MAX_SOLVER_VALUE).astype(dtype))
    assert np.all(state.beta[inf_neg] >= 0) and np.all(state.beta[inf_pos] <= 0)


def same_state(a, b):
    assert a.beta.tobytes() == b.beta.tobytes()
    assert a.resid.tobytes() == b.resid.tobytes()
    assert a.loss == b.loss and a.iters == b.iters and a.n_kkt == b.n_kkt
    assert sets_of(a) == sets_of(b)
    assert np.array_equal(a.is_screen, b.is_screen) and np.array_equal(a.is_active, b.is_active)
    assert a.grad.tobytes() == b.grad.tobytes()
    assert a.screen_AS.tobytes() == b.screen_AS.tobytes()
    assert a.screen_ASAT_diag.tobytes() == b.screen_ASAT_diag.tobytes()


def run(inputs, **kw):
    A, S, v, pneg, ppos = inputs
    return ad.pinball(np.array(A), S, v, pneg, ppos, **kw)


@pytest.mark.parametrize("m, d, kappa, pen, max_iters, seed", CASES)
def test_float64_grid(hip, m, d, kappa, pen, max_iters, seed):
    mi = MAX_ITERS if max_iters is None else max_iters
    inputs = pc.cached_inputs(m, d, seed, pen)
    own = pc.cached_run(m, d, seed, pen, kappa, "float64", max_iters=mi)
    print(f"restatement: ns {len(own.screen)}, active {len(own.active)}, iters {own.iters}, n_kkt {own.n_kkt}, exit {own.exit}, "
          f"min_gap {own.min_gap:.3e}")
    assert own.min_gap >= GAP64  # every grid case qualifies: nothing is skipped
    state = run(inputs, kappa=kappa, max_iters=mi)
    assert state.error == own.error == ("" if max_iters is None else pc.MAX_ITERS_MSG)
    assert state.beta.dtype == np.float64 and state.beta.shape == (m,) and state.resid.shape == (d,)
    check_exact(state, own)
    truth = pc.cached_run(m, d, seed, pen, kappa, "longdouble", max_iters=mi)
    assert truth.screen == own.screen and truth.active == own.active and truth.iters == own.iters
    check_close(state, own, truth, inputs, EPS64)
    check_invariants(state, inputs)
    print(f"changed visits: device {state.benchmark['n_changed']:.0f}, restatement {own.n_changed}")


def truth32(m, d, seed, pen, kappa):
    return pc.cached_run(m, d, seed, pen, kappa, "float64", True)


def test_float32_cases_qualify():
    """Skipping may not hide a failure: at most one of the nine float32 cases is too close to a decision for an exact check."""
    under = [(m, d, s) for (m, d, kappa, pen) in GRID32 for s in range(3) if truth32(m, d, s, pen, kappa).min_gap < GAP32]
    print("float32 cases under GAP32:", under)
    assert len(under) <= 1


@pytest.mark.parametrize("m, d, kappa, pen", GRID32)
@pytest.mark.parametrize("seed", range(3))
def test_float32_grid(hip, m, d, kappa, pen, seed):
    inputs = pc.cached_inputs(m, d, seed, pen, None, True)  # A, S, v rounded to float32
    truth = truth32(m, d, seed, pen, kappa)
    own = pc.cached_run(m, d, seed, pen, kappa, "float32", True)
    state = run(inputs, kappa=kappa)
    assert state.error == ""
    assert state.beta.dtype == np.float32 and state.resid.dtype == np.float32 and state.screen_AS.dtype == np.float32
    print(f"float64 restatement on the rounded inputs: min_gap {truth.min_gap:.3e}")
    if truth.min_gap >= GAP32:
        assert own.screen == truth.screen and own.active == truth.active
        check_exact(state, truth)
    check_close(state, own, truth, inputs, EPS32)
    check_invariants(state, inputs)
    same_state(state, run(inputs, kappa=kappa))


@pytest.mark.parametrize("seed", range(3))
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_edge_inputs(hip, dtype, seed):
    """Infinite penalties on either side (inf itself in float32), a zero row (v_k = 0) and a repeated row."""
    r32 = dtype == "float32"
    inputs = pc.cached_inputs("edge", 0, seed, 1.0, None, r32)
    own = pc.cached_run("edge", 0, seed, 1.0, None, dtype, r32)
    truth = pc.cached_run("edge", 0, seed, 1.0, None, "float64" if r32 else "longdouble", r32)
    print(f"restatement: ns {len(own.screen)}, min_gap {own.min_gap:.3e}; wider format: min_gap {truth.min_gap:.3e}")
    state = run(inputs)
    assert state.error == ""
    if not r32:
        assert own.min_gap >= GAP64
        check_exact(state, own)
    elif truth.min_gap >= GAP32:
        check_exact(state, truth)
    check_close(state, own, truth, inputs, EPS32 if r32 else EPS64)
    check_invariants(state, inputs)
    assert np.all(state.beta[::2] >= 0) and np.all(state.beta[1::4] <= 0)
    assert state.beta[5] == 0  # the zero row is never changed
    if r32:
        assert np.isinf(state.penalty_neg[0]) and np.isinf(state.penalty_pos[1])


def test_both_penalties_infinite(hip):
    """A coordinate that may move neither way: in float32 both clipped penalties are inf, the update gives copysign(0, inf) = 0
    and the violation is -inf (sorted last, never admitted); in float64 the same with 1e100."""
    A, S, v, pneg, ppos = (np.array(x) for x in pc.cached_inputs(20, 5, 0, 1.0))
    pneg[3] = ppos[3] = np.inf
    for dtype in (np.float32, np.float64):
        A_, S_, v_ = A.astype(dtype), np.asfortranarray(S.astype(dtype)), v.astype(dtype)
        own = pc.solve(A_, S_, v_, pneg, ppos, dtype)
        state = ad.pinball(A_, S_, v_, pneg, ppos)
        assert state.error == "" and state.beta[3] == 0 and not state.is_screen[3]
        assert state.grad[3] == own.grad[3] and (np.isneginf(state.grad[3]) if dtype == np.float32 else state.grad[3] < -1e99)
        print(f"{np.dtype(dtype).name}: violation of the pinned coordinate {state.grad[3]}, restatement min_gap {own.min_gap:.3e}")
        if own.min_gap >= (GAP32 if dtype == np.float32 else GAP64):
            check_exact(state, own)
    # pinned from the start inside a warm start's screen set: still never moved
    warm = ad.pinball(A, S, v, pneg, ppos)
    warm.active_set[warm.active_set_size] = 3
    warm.active_set_size += 1
    warm.is_active[3] = True
    again = ad.pinball(A.astype(np.float32), S, v, pneg, ppos, warm_start=warm)
    assert again.error == "" and again.beta[3] == 0 and again.is_screen[3] and not again.is_active[3]


def test_global_storage_gives_the_same_bits(hip):
    inputs = pc.cached_inputs(130, 40, 0, 0.3)
    in_lds = run(inputs)
    try:
        set_config("pinball_lds_max_ns", 1)
        in_global = run(inputs)
    finally:
        set_config("pinball_lds_max_ns", 0)
    assert in_lds.screen_set_size > 1
    same_state(in_lds, in_global)
    check_exact(in_global, pc.cached_run(130, 40, 0, 0.3, None, "float64"))


def test_rerun_gives_the_same_bits(hip):
    inputs = pc.cached_inputs(300, 64, 0, 0.1)
    same_state(run(inputs, kappa=7), run(inputs, kappa=7))


def test_gram_limit(hip):
    inputs = pc.cached_inputs(130, 40, 0, 0.3)
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
    m, d, pen = 130, 40, 0.3
    inputs = pc.cached_inputs(m, d, 0, pen)
    A, S, v, pneg, ppos = inputs
    coarse = run(inputs, tol=1e-4)
    own1 = pc.cached_run(m, d, 0, pen, None, "float64", tol=1e-4)
    truth1 = pc.cached_run(m, d, 0, pen, None, "longdouble", tol=1e-4)
    assert own1.min_gap >= GAP64
    check_exact(coarse, own1)
    fine = run(inputs, tol=1e-9, warm_start=coarse)
    own2 = pc.solve(A, S, v, pneg, ppos, np.float64, tol=1e-9, warm_start=own1)
    truth2 = pc.solve(A, S, v, pneg, ppos, np.longdouble, tol=1e-9, warm_start=truth1)
    print(f"warm restatement: ns {len(own2.screen)}, iters {own2.iters}, n_kkt {own2.n_kkt}, min_gap {own2.min_gap:.3e}")
    assert fine.error == "" and own2.min_gap >= GAP64
    check_exact(fine, own2)
    check_close(fine, own2, truth2, inputs, EPS64)
    check_invariants(fine, inputs)
    again = run(inputs, tol=1e-9, warm_start=fine)
    assert again.error == "" and again.screen_set_size == fine.active_set_size  # no admissions from the solution
    assert sets_of(again)[0] == sets_of(fine)[1]


def test_input_forms(hip):
    import torch

    inputs = pc.cached_inputs(130, 40, 1, 0.3)
    A, S, v, pneg, ppos = inputs
    base = ad.pinball(np.ascontiguousarray(A), S, v, pneg, ppos)
    same_state(base, ad.pinball(np.asfortranarray(A), S, v, pneg, ppos))
    t = torch.from_numpy(np.array(A, order="C")).to("cuda")
    same_state(base, ad.pinball(t, S, v, pneg, ppos))
    same_state(base, ad.pinball(t.t().contiguous().t(), S, v, pneg, ppos))  # F-contiguous on the device
    M = ad.matrix.dense(t, method="constraint")
    assert isinstance(M, ad.matrix.MatrixConstraintBase64) and M.shape == (130, 40)
    same_state(base, ad.pinball(M, S, v, pneg, ppos))


@pytest.mark.parametrize("m, d", [(37, 1), (5, 70), (300, 33)])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_constraint_matrix_operations(hip, m, d, dtype):
    """Against numpy in float64; the bound is k eps sum |a| |b| per dot of k terms (nested dots add their terms)."""
    rs = np.random.RandomState(m + d)
    A = rs.normal(size=(m, d)).astype(dtype)
    eps = float(np.finfo(dtype).eps)
    A64, aA = A.astype(np.float64), np.abs(A.astype(np.float64))
    for order in ("C", "F"):
        M = ad.matrix.dense(np.array(A, order=order), method="constraint")
        assert isinstance(M, ad.matrix.MatrixConstraintBase64 if dtype == np.float64 else ad.matrix.MatrixConstraintBase32)
        assert (M.rows(), M.cols(), M.shape, M.ndim) == (m, d, (m, d), 2)
        assert np.array_equal(M.to_dense(), A)
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
        val = rs.normal(size=idx.size).astype(dtype)
        M.sp_mul(idx, val, out)
        close(out, val.astype(np.float64) @ A64[idx], (idx.size + 1) * eps * (np.abs(val.astype(np.float64)) @ aA[idx]), "sp_mul")
        j = m // 2
        M.rmmul(j, Q, out)
        close(out, A64[j] @ Q64, (d + 1) * eps * (aA[j] @ np.abs(Q64)), "rmmul")
        M.rmmul_safe(j, Q, out)
        close(out, A64[j] @ Q64, (d + 1) * eps * (aA[j] @ np.abs(Q64)), "rmmul_safe")
        for f in (M.rvmul, M.rvmul_safe):
            close(f(j, v), A64[j] @ v64, (d + 1) * eps * (aA[j] @ np.abs(v64)), "rvmul")
        start = rs.normal(size=d).astype(dtype)
        out = start.copy()
        M.rvtmul(j, dtype(0.75), out)
        close(out, start.astype(np.float64) + 0.75 * A64[j], 2 * eps * (np.abs(start.astype(np.float64)) + 0.75 * aA[j]), "rvtmul")
        C = np.empty((m, m), dtype=dtype)
        M.cov(Q, C)
        close(C, A64 @ Q64 @ A64.T, (2 * d + 2) * eps * (aA @ np.abs(Q64) @ aA.T), "cov")
        print(f"({m}, {d}) {np.dtype(dtype).name} {order}: worst error / bound {worst:.3f}")


def test_naive_entry_points_refuse_a_constraint_matrix(hip):
    A, S, v, pneg, ppos = pc.cached_inputs(20, 5, 0, 1.0)
    M = ad.matrix.dense(np.array(A), method="constraint")
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
    # the core refuses the handle itself, in the words of its covariance refusals
    b = M._backend
    out = np.zeros(20)
    ones = np.ones(5)
    assert b.fn("design_mul")(M._handle, ones.ctypes.data, ones.ctypes.data, out.ctypes.data) != 0
    assert "not a constraint matrix" in b.fn("last_error")().decode()
    handle = _abi.C.c_void_p()
    assert b.fn("design_alias")(M._handle, handle) != 0
    assert "not a constraint matrix" in b.fn("last_error")().decode()
    D = ad.matrix.dense(np.asfortranarray(A))
    with pytest.raises(ValueError, match="MatrixConstraintBase"):
        ad.state.pinball(A=D, y_var=1.0, S=S, penalty_neg=pneg, penalty_pos=ppos, kappa=1, max_iters=10, tol=1e-7,
                         screen_set_size=0, screen_set=np.zeros(20, dtype=int), is_screen=np.zeros(20, dtype=bool),
                         screen_ASAT_diag=None, screen_AS=None, active_set_size=0, active_set=np.zeros(20, dtype=int),
                         is_active=np.zeros(20, dtype=bool), beta=np.zeros(20), resid=v, grad=np.zeros(20), loss=0.5)


def test_core_validation(hip):
    """The C entry repeats state_pinball.ipp's checks and adds its own on the sets."""
    A, S, v, pneg, ppos = pc.cached_inputs(20, 5, 0, 1.0)
    M = ad.matrix.dense(np.array(A), method="constraint")
    b = M._backend
    m, d = 20, 5
    Sf = np.asfortranarray(S)
    beta, grad, resid = np.zeros(m), np.zeros(m), np.array(v)
    screen = np.array([3, 3], dtype=np.int64)

    def call(**change):
        kw = dict(S=_abi.ptr(Sf), penalty_neg=_abi.ptr(pneg), penalty_pos=_abi.ptr(ppos), beta=_abi.ptr(beta), resid=_abi.ptr(resid),
                  grad=_abi.ptr(grad), S_rows=d, S_cols=d, n_penalty_neg=m, n_penalty_pos=m, n_beta=m, n_resid=d, n_grad=m,
                  screen_set=None, screen_set_size=0, active_set=None, active_set_size=0, n_screen_set=m, n_is_screen=m,
                  n_active_set=m, n_is_active=m, n_screen_ASAT_diag=m, screen_AS_rows=m, screen_AS_cols=d, y_var=1.0, loss=0.5,
                  kappa=2, max_iters=100, tol=1e-7)
        kw.update(change)
        handle = _abi.C.c_void_p()
        rc = b.fn("pinball_solve")(M._handle, _abi.C.byref(_abi.PinballArgs(**kw)), handle)
        if rc == 0:
            b.fn("pinball_result_destroy")(handle)
            return ""
        return b.fn("last_error")().decode()

    assert call() == ""
    assert call(S_rows=4) == "adelie_core solver: S must be (d, d) where A is (m, d). "
    assert call(n_resid=4) == "adelie_core solver: resid must be (d,) where A is (m, d). "
    assert call(kappa=0) == "adelie_core solver: kappa must be > 0. "
    assert call(screen_AS_cols=4) == "adelie_core solver: screen_AS must be (m, d) where A is (m, d). "
    assert call(screen_set=_abi.ptr(screen), screen_set_size=2) == "adelie_core: pinball: screen_set must hold distinct indices in [0, m)."
    assert call(active_set=_abi.ptr(screen), active_set_size=1) == "adelie_core: pinball: active_set must hold distinct members of screen_set."


def test_python_route_on_the_device_matrix(hip, monkeypatch):
    """The resident matrix forced through the Python route (its rvmul / rmmul / tmul, one device call each) reaches the native
    route's trajectory."""
    inputs = pc.cached_inputs(20, 5, 0, 1.0)
    native = run(inputs)
    monkeypatch.setattr(ad.state, "_pinball_native", lambda A: False)
    routed = run(inputs)
    assert routed.error == "" and routed.benchmark.keys() == {"n_changed"}
    assert sets_of(routed) == sets_of(native) and (routed.iters, routed.n_kkt) == (native.iters, native.n_kkt)
    own = pc.cached_run(20, 5, 0, 1.0, None, "float64")
    check_exact(routed, own)
    check_close(routed, own, pc.cached_run(20, 5, 0, 1.0, None, "longdouble"), inputs, EPS64)
