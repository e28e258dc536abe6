"""Box / one-sided constraint objects on groups of 65 to 128 coefficients, solved on the device (kernels_cons_wide.hip): one visit
through adelie_hip_cons_visit_test against the KKT system of the group problem in extended precision, with the host object's own
KKT residual as the yardstick, and a path whose wide groups must not visit the host."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import adelie_amd as ad
from adelie_amd import _abi, constraint

CFG = {"max_iters": 1000, "tol": 1e-14, "pinball_max_iters": 1000000, "pinball_tol": 1e-13}  # (test_constraint.py:840)
SEEDS = {"far": 11, "bind": 12, "inside": 13, "absorb": 14}
L2 = 0.1
FAR = 1e3


@functools.lru_cache(maxsize=None)
def _case(native, d, dtype, kind):
    """The inputs of one visit, and the host object's solution of it (computed once)."""
    rng = np.random.RandomState(1000 * SEEDS[kind] + d + (native == "box"))
    Q = np.asfortranarray(np.linalg.qr(rng.randn(d, d))[0].astype(dtype))
    quad = rng.uniform(0.5, 2.0, d).astype(dtype)
    lin0 = rng.randn(d) * 3.0
    sgn = np.where(rng.rand(d) < 0.5, -1.0, 1.0)
    l1 = 0.5
    x0 = np.zeros(d)
    z = Q.astype(float) @ (lin0 / (quad + L2))  # about where the unconstrained solution lies, in the constraint's coordinates
    lo, up, b = np.full(d, -FAR), np.full(d, FAR), np.full(d, FAR)
    if kind == "bind":  # a good share of the coordinates held back to 0.3 of where they want to be, from a non-zero start
        tight = rng.rand(d) < 0.4
        up = np.where(tight & (z > 0), 0.3 * np.abs(z), FAR)
        lo = np.where(tight & (z < 0), -0.3 * np.abs(z), -FAR)
        b = np.where(tight & (sgn * z > 0), 0.3 * np.abs(z), FAR)
        x0 = 0.1 * rng.randn(d)
    elif kind == "inside":
        l1 = 1.5 * np.linalg.norm(lin0)
        x0 = 0.1 * rng.randn(d)
    elif kind == "absorb":  # bounds at 0 on a share of the coordinates; l1 just above what their multipliers cannot absorb
        zero = rng.rand(d) < 0.8
        lo, up, b = np.where(zero, 0.0, -FAR), np.where(zero, 0.0, FAR), np.where(zero, 0.0, FAR)
    beta = (Q.astype(float) @ x0).astype(dtype)
    grad = (Q.astype(float) @ (lin0 - quad * x0)).astype(dtype)
    # what the visit itself forms from its arrays: linear = grad V + vars * (beta V), the start beta V
    Qd = Q.astype(float)
    x0 = beta.astype(float) @ Qd
    lin = grad.astype(float) @ Qd + quad.astype(float) * x0
    va, vb = (lo, up) if native == "box" else (sgn, b)
    va, vb = va.astype(dtype), vb.astype(dtype)
    if kind == "absorb":
        Qv = Qd @ lin
        mu = np.clip(Qv, np.where(va >= 0, -1e100, 0), np.where(vb <= 0, 1e100, 0)) if native == "box" else \
            va * np.minimum(np.maximum(va * Qv, 0), np.where(vb <= 0, 1e100, 0))
        l1 = 1.05 * np.linalg.norm(Qv - mu)
        assert l1 < 0.98 * np.linalg.norm(lin)
    obj = (constraint.box(va.astype(float), vb.astype(float), configs=CFG) if native == "box"
           else constraint.one_sided(va.astype(float), vb.astype(float), configs=CFG))
    xh = x0.copy()
    obj.solve(xh, quad.astype(float), lin, l1, L2, Qd)  # (raises unless the object ends with status OK)
    return dict(Q=Q, quad=quad, grad=grad, beta=beta, va=va, vb=vb, l1=float(l1), lin=lin, xh=xh, muh=obj._mu.astype(float).copy())


def _kkt(native, c, x, mu):
    """KKT residual of  min 1/2 x'diag(quad)x - lin'x + l1|x| + 1/2 l2|x|^2  s.t.  lo <= Qx <= up  (one-sided: sgn o Qx <= b),
    in numpy.longdouble: stationarity, primal feasibility, the signs of mu, complementary slackness."""
    L = np.longdouble
    Q, quad, lin, va, vb = (np.asarray(c[k], dtype=L) for k in ("Q", "quad", "lin", "va", "vb"))
    x, mu, l1 = np.asarray(x, dtype=L), np.asarray(mu, dtype=L), L(c["l1"])
    z = Q @ x
    g = (mu if native == "box" else va * mu) @ Q  # Q'A'mu
    nx = np.sqrt(np.sum(x * x))
    if nx > 0:
        stat = np.abs((quad + L(L2)) * x - lin + l1 * x / nx + g).max()
    else:
        stat = max(np.sqrt(np.sum((lin - g) ** 2)) - l1, L(0))
    if native == "box":
        feas = max((z - vb).max(), (va - z).max(), L(0))
        sign = L(0)  # (mu = mu_+ - mu_-: either sign is a multiplier, of the side complementary slackness names)
        slack = max(np.abs(np.maximum(mu, 0) * (vb - z)).max(), np.abs(np.maximum(-mu, 0) * (z - va)).max())
    else:
        feas = max((va * z - vb).max(), L(0))
        sign = max((-mu).max(), L(0))
        slack = np.abs(mu * (va * z - vb)).max()
    return float(max(stat, feas, sign, slack))


def _visit(hip, native, c, dtype, gram):
    d = len(c["quad"])
    beta, mu = c["beta"].copy(), np.zeros(d, dtype=dtype)
    dcol, dlt = np.full(d, -1, dtype=np.int32), np.zeros(d, dtype=dtype)
    st_f, st_i = np.zeros(4), np.zeros(5, dtype=np.int64)
    a = _abi.ConsVisit(dtype=_abi.dtype_code(dtype), q=d, native=4 if native == "box" else 5, gram=int(gram), mark=1,
                       first_of_pass=1, max_active_size=8, col0=7, l1=c["l1"], l2=L2, dbeta_tol=0.0)
    cfg = dict(constraint._PROX_NEWTON_DEFAULTS, **CFG)
    a.cfg[:] = [cfg[k] for k in ("max_iters", "tol", "pinball_max_iters", "pinball_tol", "slack")]
    for name, arr in (("V", c["Q"]), ("grad", c["grad"]), ("beta", beta), ("vars", c["quad"]), ("va", c["va"]), ("vb", c["vb"]),
                      ("mu", mu), ("dcol", dcol), ("dlt", dlt), ("st_f", st_f), ("st_i", st_i)):
        setattr(a, name, arr.ctypes.data)
    hip.check(hip.fn("cons_visit_test")(C.byref(a)))
    return beta, mu, dcol, dlt, st_f, st_i


PARAMS = [(nat, d, np.float64) for nat in ("box", "one_sided") for d in (65, 127, 128)] + [("box", 128, np.float32)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(SEEDS))
@pytest.mark.parametrize("native,d,dtype", PARAMS)
def test_one_wide_visit_against_the_kkt_system(hip, native, d, dtype, kind):
    c = _case(native, d, dtype, kind)
    f32 = dtype == np.float32
    Qd = c["Q"].astype(float)
    beta, mu, dcol, dlt, st_f, st_i = _visit(hip, native, c, dtype, gram=False)
    again = _visit(hip, native, c, dtype, gram=False)
    assert st_i[2] == 0, st_i  # status OK
    assert all(np.array_equal(u.view(np.uint8), v.view(np.uint8)) for u, v in zip((beta, mu, dcol, dlt, st_f[:3], st_i), again[:4] + (again[4][:3], again[5])))
    x = beta.astype(float) @ Qd
    host, dev = _kkt(native, c, c["xh"], c["muh"]), _kkt(native, c, x, mu)
    # the device gets four times the host object's own residual (the two sum in different orders and stop on the same rule); the
    # floor is what the rounding of a d-term sum of values of the size of `linear` leaves in the format the results are stored in
    floor = d * float(np.finfo(dtype).eps) * max(1.0, float(np.linalg.norm(c["lin"])))
    print(f"cons_wide visit {native} d={d} {np.dtype(dtype).name} {kind}: kkt device {dev:.3e} host {host:.3e} "
          f"ratio {dev / host if host > 0 else float('inf'):.3g} floor {floor:.3e} ms {st_f[3]:.4f}")
    assert dev <= 4 * host + floor, (dev, host, floor)
    assert np.abs(x - c["xh"]).max() < (2e-3 if f32 else 1e-7)
    if kind == "far":
        assert np.all(mu == 0) and np.any(x != 0)
    elif kind == "bind":
        z = Qd @ x
        gap = np.minimum(c["vb"] - z, z - c["va"]) if native == "box" else c["vb"] - c["va"] * z
        assert np.any(mu != 0) and np.any(np.abs(gap) < (1e-3 if f32 else 1e-7))
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
    from util import make_gaussian

    sizes = np.array([65, 128, 96, 8, 1, 1, 1])
    groups = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    d = make_gaussian(300, 300, seed=3, sparsity=0.5, dtype=dtype)

    def make():  # (a list per fit: the objects keep state)
        r = np.random.RandomState(5)
        return [constraint.lower(np.zeros(65), dtype=dtype), constraint.lower(np.zeros(128), dtype=dtype),
                constraint.box(-r.uniform(0.02, 0.2, 96), r.uniform(0.02, 0.2, 96), dtype=dtype),
                constraint.one_sided(np.where(r.rand(8) < 0.5, -1.0, 1.0), r.uniform(0.02, 0.2, 8), dtype=dtype),
                None, None, None]

    return d, groups, make


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["naive64", "naive32", "cov64"])
def test_wide_groups_stay_on_the_device_along_a_path(hip, oracle, route):
    dtype = np.float32 if route == "naive32" else np.float64
    f32 = dtype == np.float32
    d, groups, make = _path_problem(dtype)
    X, y, n = d["X"], d["y"], 300
    kw = dict(groups=groups, alpha=0.7, lmda_path_size=8, min_ratio=0.05, early_exit=False, tol=1e-7 if f32 else 1e-13,
              progress_bar=False)
    if f32:
        kw["newton_tol"] = 1e-5  # (test_constraint.py:676)
    if route == "cov64":
        Xc, yc = X - X.mean(axis=0), y - y.mean()
        A, v = np.asfortranarray(Xc.T @ Xc / n), Xc.T @ yc / n
        fit = lambda dense, cons: ad.gaussian_cov(dense(A), v, constraints=cons, **kw)
        dev_m, ref_m = (lambda M: ad.matrix.dense(M, method="cov")), oracle.cov_dense
    else:
        fit = lambda dense, cons: ad.grpnet(dense(X), ad.glm.gaussian(y, dtype=dtype), constraints=cons, **kw)
        dev_m, ref_m = ad.matrix.dense, oracle.dense
    ref = fit(ref_m, make())
    assert ref.error == "" and len(ref.lmdas) == 8
    # the problem exercises what it is here for: every wide group screened, one of them active against a bound
    dg, Rd, Rb = np.asarray(ref.dual_groups), ref.duals.toarray(), ref.betas.toarray()
    assert all(g in set(ref.screen_set) for g in (0, 1, 2))
    assert any(np.any(Rd[:, dg[g]:dg[g] + s] != 0) and np.any(Rb[:, groups[g]:groups[g] + s] != 0) for g, s in ((0, 65), (1, 128), (2, 96)))
    st = fit(dev_m, make())
    assert st.error == "" and len(st.lmdas) == len(ref.lmdas)
    tol = 2e-3 if f32 else 1e-7
    B = st.betas.toarray()
    assert np.abs(B - Rb).max() < tol
    assert st.duals.shape == ref.duals.shape and ref.duals.nnz > 0
    dscale = max(1.0, float(np.abs(ref.duals).max()))
    assert np.abs((st.duals - ref.duals)).max() < (2e-2 if f32 else 1e-5) * dscale
    assert np.abs(st.abs_grad - ref.abs_grad).max() < (1e-2 if f32 else 1e-6)
    if not f32:
        assert np.array_equal(np.sort(st.screen_set), np.sort(ref.screen_set))
    assert st.counters["n_host_cons_visits"] == 0 and st.counters["n_dev_cons_visits"] > 0, st.counters
    os.environ["ADELIE_HIP_CONS_HOST"] = "1"
    try:
        sth = fit(dev_m, make())
    finally:
        del os.environ["ADELIE_HIP_CONS_HOST"]
    assert sth.error == "" and sth.counters["n_dev_cons_visits"] == 0 and sth.counters["n_host_cons_visits"] > 0
    assert np.abs(sth.betas.toarray() - B).max() < tol
    assert np.abs((sth.duals - st.duals)).max() < (2e-2 if f32 else 1e-5) * dscale
