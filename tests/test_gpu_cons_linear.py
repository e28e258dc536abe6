"""`linear` constraint objects (lower <= A x <= upper, m rows on d coefficients, both <= 64) solved on the device
(kernels_cons_linear.hip): one visit through adelie_hip_cons_visit_test against the KKT system of the group problem in extended
precision, with the host object's own KKT residual as the yardstick, and paths whose linear groups must not visit the host."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import adelie_amd as ad
from adelie_amd import _abi, constraint

TIGHT = {"tol": 1e-13, "pinball_tol": 1e-12, "nnls_tol": 1e-12, "max_iters": 1000}  # (test_constraint.py:936)
SEEDS = {"far": 21, "bind": 22, "inside": 23, "absorb": 24}
L2 = 0.1
FAR = 1e3


@functools.lru_cache(maxsize=None)
def _case(m, d, dtype, kind):
    """The inputs of one visit, and the host object's solution of it (computed once)."""
    rng = np.random.RandomState(1000 * SEEDS[kind] + 64 * m + d)
    Q = np.asfortranarray(np.linalg.qr(rng.randn(d, d))[0].astype(dtype))
    quad = rng.uniform(0.5, 2.0, d).astype(dtype)
    lin0 = rng.randn(d) * 3.0
    A = rng.randn(m, d) / np.sqrt(d)
    l1 = 0.5
    x0 = np.zeros(d)
    w = A @ (Q.astype(float) @ (lin0 / (quad + L2)))  # about where A Q x wants to be without the constraint
    lo, up = np.full(m, -FAR), np.full(m, FAR)
    if kind == "bind":  # a share of the rows held back to 0.3 of where they want to be, from a non-zero start
        tight = rng.rand(m) < 0.4
        tight[np.argmax(np.abs(w))] = True
        up = np.where(tight & (w > 0), 0.3 * np.abs(w), FAR)
        lo = np.where(tight & (w < 0), -0.3 * np.abs(w), -FAR)
        x0 = 0.1 * rng.randn(d)
    elif kind == "inside":
        l1 = 1.5 * np.linalg.norm(lin0)
        x0 = 0.1 * rng.randn(d)
    elif kind == "absorb":  # bounds at 0 on most rows; l1 just above what their multipliers cannot absorb
        zero = rng.rand(m) < 0.8
        zero[0] = True
        lo, up = np.where(zero, 0.0, -FAR), np.where(zero, 0.0, FAR)
    Qd = Q.astype(float)
    beta = (Qd @ x0).astype(dtype)
    grad = (Qd @ (lin0 - quad * x0)).astype(dtype)
    # what the visit itself forms from its arrays: linear = grad V + vars * (beta V), the start beta V
    x0 = beta.astype(float) @ Qd
    lin = grad.astype(float) @ Qd + quad.astype(float) * x0
    if kind == "absorb":  # (a row bound at 0 on both sides has a multiplier of either sign, every other row none at x = 0)
        Az, Qv = A[zero].T, Qd @ lin
        rest, full = np.linalg.norm(Qv - Az @ np.linalg.lstsq(Az, Qv, rcond=None)[0]), np.linalg.norm(lin)
        l1 = rest + 0.25 * (full - rest)
    obj = constraint.linear(A, lo, up, configs=TIGHT)
    xh = x0.copy()
    obj.solve(xh, quad.astype(float), lin, l1, L2, Qd)  # (raises unless the object ends with status OK)
    return dict(Q=Q, quad=quad, grad=grad, beta=beta, A=A, lo=lo, up=up, vars=obj._vars.copy(), l1=float(l1), lin=lin, xh=xh,
                muh=obj._mu.astype(float).copy())


def _kkt(c, x, mu):
    """KKT residual of  min 1/2 x'diag(quad)x - lin'x + l1|x| + 1/2 l2|x|^2  s.t.  lo <= A Q x <= up  in numpy.longdouble:
    stationarity with Q'A'mu, primal feasibility, complementary slackness per side."""
    L = np.longdouble
    Q, quad, lin, A, lo, up = (np.asarray(c[k], dtype=L) for k in ("Q", "quad", "lin", "A", "lo", "up"))
    x, mu, l1 = np.asarray(x, dtype=L), np.asarray(mu, dtype=L), L(c["l1"])
    z = A @ (Q @ x)
    g = (mu @ A) @ Q  # Q'A'mu
    nx = np.sqrt(np.sum(x * x))
    if nx > 0:
        stat = np.abs((quad + L(L2)) * x - lin + l1 * x / nx + g).max()
    else:
        stat = max(np.sqrt(np.sum((lin - g) ** 2)) - l1, L(0))
    feas = max((z - up).max(), (lo - z).max(), L(0))
    slack = max(np.abs(np.maximum(mu, 0) * (up - z)).max(), np.abs(np.maximum(-mu, 0) * (z - lo)).max())
    return float(max(stat, feas, slack))


def _visit(hip, c, dtype):
    m, d = c["A"].shape
    beta, mu = c["beta"].copy(), np.zeros(m, dtype=dtype)
    dcol, dlt = np.full(d, -1, dtype=np.int32), np.zeros(d, dtype=dtype)
    order, norder = np.full(m, -1, dtype=np.int32), np.zeros(1, dtype=np.int32)
    st_f, st_i = np.zeros(4), np.zeros(5, dtype=np.int64)
    a = _abi.ConsVisit(dtype=_abi.dtype_code(dtype), q=d, m=m, native=constraint.NATIVE_LINEAR, mark=1, first_of_pass=1,
                       max_active_size=8, col0=7, l1=c["l1"], l2=L2, dbeta_tol=0.0)
    cfg = dict(constraint._PROX_NEWTON_DEFAULTS, **TIGHT)
    a.cfg[:] = [cfg[k] for k in ("max_iters", "tol", "pinball_max_iters", "pinball_tol", "slack")]
    a.lin_cfg[:] = [1e5, TIGHT["nnls_tol"]]
    for name, arr in (("V", c["Q"]), ("grad", c["grad"]), ("beta", beta), ("vars", c["quad"]), ("mu", mu), ("dcol", dcol),
                      ("dlt", dlt), ("st_f", st_f), ("st_i", st_i), ("lin_A", c["A"]), ("lin_lower", c["lo"]), ("lin_upper", c["up"]),
                      ("lin_vars", c["vars"]), ("lin_order", order), ("lin_norder", norder)):
        setattr(a, name, arr.ctypes.data)
    hip.check(hip.fn("cons_visit_test")(C.byref(a)))
    return beta, mu, dcol, dlt, order, norder, st_f, st_i


SHAPES = [(1, 2), (3, 2), (5, 8), (17, 16), (16, 17), (64, 64), (64, 3), (2, 64)]
PARAMS = [(m, d, np.float64) for m, d in SHAPES] + [(64, 64, np.float32)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(SEEDS))
@pytest.mark.parametrize("m,d,dtype", PARAMS)
def test_one_linear_visit_against_the_kkt_system(hip, m, d, dtype, kind):
    c = _case(m, d, dtype, kind)
    f32 = dtype == np.float32
    Qd = c["Q"].astype(float)
    beta, mu, dcol, dlt, order, norder, st_f, st_i = _visit(hip, c, dtype)
    again = _visit(hip, c, dtype)
    assert st_i[2] == 0, st_i  # status OK
    assert all(np.array_equal(u.view(np.uint8), v.view(np.uint8))
               for u, v in zip((beta, mu, dcol, dlt, order, norder, st_f[:3], st_i), again[:6] + (again[6][:3], again[7])))
    x = beta.astype(float) @ Qd
    host, dev = _kkt(c, c["xh"], c["muh"]), _kkt(c, x, mu)
    # the device gets four times the host object's own residual (the two sum in different orders and stop on the same rule); the
    # floor is what the rounding of a max(m, d)-term sum of values of the size of `linear` leaves in the format the results are
    # stored in (test_gpu_cons_wide.py:120-126)
    floor = max(m, d) * float(np.finfo(dtype).eps) * max(1.0, float(np.linalg.norm(c["lin"])))
    print(f"cons_linear visit m={m} d={d} {np.dtype(dtype).name} {kind}: kkt device {dev:.3e} host {host:.3e} "
          f"ratio {dev / host if host > 0 else float('inf'):.3g} floor {floor:.3e} ms {st_f[3]:.4f}")
    assert dev <= 4 * host + floor, (dev, host, floor)
    tol = 2e-3 if f32 else 1e-7
    assert np.abs(x - c["xh"]).max() < tol
    if np.any(x != 0):
        assert np.abs(c["A"].T @ (mu.astype(float) - c["muh"])).max() < tol
    if m <= d:
        assert np.abs(mu - c["muh"]).max() < tol
    nz = np.flatnonzero(np.abs(mu) > 1e-16)
    assert norder[0] == len(nz) and sorted(order[:norder[0]]) == list(nz) and np.all(order[norder[0]:] == -1)
    if kind == "far":
        assert np.all(mu == 0) and np.any(x != 0)
    elif kind == "bind":
        z = c["A"] @ (Qd @ x)
        assert np.any(mu != 0) and np.any(np.abs(np.minimum(c["up"] - z, z - c["lo"])) < (1e-3 if f32 else 1e-7))
    elif kind == "inside":
        assert np.all(beta == 0) and np.all(mu == 0)
    else:
        assert np.all(beta == 0) and np.any(mu != 0)
    if st_i[3]:  # the group changed: the change list and the pass state of a first visit
        assert st_i[3] == d and st_i[0] == 1 and st_i[1] == 1 and st_i[4] == 1
        assert np.array_equal(dcol, 7 + np.arange(d)) and np.array_equal(dlt, beta - c["beta"])
    else:
        assert st_i[0] == 0 and st_i[1] == 0 and np.all(dcol == -1)


def _path_problem(dtype):
    """Groups of 4 on a 300 x 60 design, every other one with a linear object of 1 to 5 rows (test_constraint.py:902-912);
    make(wide=True) adds one of 65 rows on the last of them: that one stays on the host."""
    from util import make_gaussian

    d = make_gaussian(300, 60, seed=14, sparsity=0.7, dtype=dtype)
    rng = np.random.RandomState(4)
    groups = np.arange(0, 60, 4)
    spec = []
    for g in range(len(groups)):
        m = rng.randint(1, 6) if g < 14 else 65
        spec.append(None if g % 2 else (rng.randn(m, 4), -rng.uniform(0, 0.2, m) * (rng.rand(m) < 0.7), rng.uniform(0.02, 0.2, m)))
    make = lambda wide=False: [None if s is None or (g == 14 and not wide) else constraint.linear(*s, configs=TIGHT, dtype=dtype)
                               for g, s in enumerate(spec)]  # (a list per fit: the objects keep state)
    return d, groups, make


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["naive64", "naive32", "cov64"])
def test_linear_groups_stay_on_the_device_along_a_path(hip, oracle, route):
    dtype = np.float32 if route == "naive32" else np.float64
    f32 = dtype == np.float32
    d, groups, make = _path_problem(dtype)
    X, y, n = d["X"], d["y"], 300
    kw = dict(groups=groups, alpha=0.8, lmda_path_size=10, min_ratio=0.05, early_exit=False, tol=1e-7 if f32 else 1e-10,
              progress_bar=False)
    if f32:
        kw["newton_tol"] = 1e-5  # (test_constraint.py:676)
    if route == "cov64":
        Xc, yc = X - X.mean(axis=0), y - y.mean()
        A, v = np.asfortranarray(Xc.T @ Xc / n), Xc.T @ yc / n
        fit = lambda dense, cons, **k: ad.gaussian_cov(dense(A), v, constraints=cons, **dict(kw, **k))
        dev_m, ref_m = (lambda M: ad.matrix.dense(M, method="cov")), oracle.cov_dense
    else:
        fit = lambda dense, cons, **k: ad.grpnet(dense(X), ad.glm.gaussian(y, dtype=dtype), constraints=cons, **dict(kw, **k))
        dev_m, ref_m = ad.matrix.dense, oracle.dense
    ref = fit(ref_m, make())
    assert ref.error == "" and len(ref.lmdas) == 10
    st = fit(dev_m, make())
    assert st.error == "" and len(st.lmdas) == len(ref.lmdas)
    assert st.counters["n_host_cons_visits"] == 0 and st.counters["n_dev_cons_visits"] > 0, st.counters
    stw = fit(dev_m, make(wide=True))  # a group with 65 rows stays on the host and is counted there
    assert stw.error == "" and stw.counters["n_host_cons_visits"] > 0 and stw.counters["n_dev_cons_visits"] > 0, stw.counters
    tol = 2e-3 if f32 else 1e-6
    B, Rb = st.betas.toarray(), ref.betas.toarray()
    assert np.abs(B - Rb).max() < tol
    assert st.duals.shape == ref.duals.shape and ref.duals.nnz > 0
    dscale = max(1.0, float(np.abs(ref.duals).max()))
    assert np.abs((st.duals - ref.duals)).max() < (2e-2 * dscale if f32 else 1e-5)
    assert np.abs(st.abs_grad - ref.abs_grad).max() < (1e-2 if f32 else 1e-6)  # (solve_zero on the unscreened groups)
    os.environ["ADELIE_HIP_CONS_HOST"] = "1"
    try:
        sth = fit(dev_m, make())
    finally:
        del os.environ["ADELIE_HIP_CONS_HOST"]
    assert sth.error == "" and sth.counters["n_dev_cons_visits"] == 0 and sth.counters["n_host_cons_visits"] > 0
    assert np.abs(sth.betas.toarray() - B).max() < tol
    assert np.abs((sth.duals - st.duals)).max() < (2e-2 * dscale if f32 else 1e-5)
    # warm start from the fifth solution with the same objects: the cold path's tail
    lm = np.asarray(st.lmdas)
    cw = make()
    head = fit(dev_m, cw, lmda_path=lm[:5])
    rest = fit(dev_m, cw, warm_start=head, lmda_path=lm[5:])
    assert rest.error == "" and np.abs(rest.betas.toarray() - B[5:]).max() < tol
