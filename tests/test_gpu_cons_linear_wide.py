"""`linear` constraint objects (m <= 64 rows) on groups of 65 to 128 coefficients, solved on the device by one workgroup
(kernels_cons_linear_wide.hip): the checks of test_gpu_cons_linear.py, with its cases, KKT system and yardstick, at the smallest
shapes at which the wide kernel can go wrong, and a path whose wide linear groups must not visit the host."""
import os

import numpy as np
import pytest

import adelie_amd as ad
from adelie_amd import constraint
from test_gpu_cons_linear import SEEDS, TIGHT, _case, _kkt, _visit

# first size of the path with one row / full rows and one component in the second half / ragged tiles both ways / odd d with a
# partial last tile / the largest shape / few rows on the widest group
SHAPES = [(1, 65), (64, 65), (17, 96), (64, 127), (64, 128), (3, 128)]
PARAMS = [(m, d, np.float64) for m, d in SHAPES] + [(64, 128, np.float32)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(SEEDS))
@pytest.mark.parametrize("m,d,dtype", PARAMS)
def test_one_wide_linear_visit_against_the_kkt_system(hip, m, d, dtype, kind):
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
    # the yardstick of test_gpu_cons_linear.py: four times the host object's own residual plus the rounding floor of the format
    floor = max(m, d) * float(np.finfo(dtype).eps) * max(1.0, float(np.linalg.norm(c["lin"])))
    print(f"cons_linear_wide visit m={m} d={d} {np.dtype(dtype).name} {kind}: kkt device {dev:.3e} host {host:.3e} "
          f"floor {floor:.3e} ms {st_f[3]:.4f}")
    assert dev <= 4 * host + floor, (dev, host, floor)
    tol = 2e-3 if f32 else 1e-7
    assert np.abs(x - c["xh"]).max() < tol
    if np.any(x != 0):
        assert np.abs(c["A"].T @ (mu.astype(float) - c["muh"])).max() < tol
    assert np.abs(mu - c["muh"]).max() < tol  # (m <= d in every case here: the multipliers are unique)
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


SIZES, ROWS = np.array([65, 128, 96, 4, 1, 1]), (3, 64, 17)
GROUPS = np.concatenate([[0], np.cumsum(SIZES)[:-1]])


def _path_constraints(dtype, zero_rows):
    """Linear objects of 3 / 64 / 17 rows on the three wide groups (a list per fit: the objects keep state).  zero_rows: three
    lower bounds in ten are 0, so that those rows can hold a multiplier while the group is at zero."""
    r = np.random.RandomState(6)
    cons = []
    for m, s in zip(ROWS, SIZES):
        A, lo, at_zero, up = r.randn(m, s) / np.sqrt(s), -r.uniform(0.02, 0.2, m), r.rand(m) < 0.3, r.uniform(0.02, 0.2, m)
        cons.append(constraint.linear(A, np.where(at_zero & zero_rows, 0.0, lo), up, configs=TIGHT, dtype=dtype))
    return cons + [None, None, None]


@pytest.mark.gpu
@pytest.mark.parametrize("route,zero_rows", [("naive64", False), ("naive32", False), ("cov64", False), ("naive64", True), ("cov64", True)])
def test_wide_linear_groups_stay_on_the_device_along_a_path(hip, oracle, route, zero_rows):
    """The three routes run with every bound off zero.  A group at zero whose rows are bounded at 0 has no unique multipliers
    (0, as a visit of a screened group with |v| <= l1 leaves them, and the bounded-least-squares fit of solve_zero both satisfy
    the KKT system), so which of them the duals report depends on whether the group was screened at that lambda, and float32
    screens differ from the oracle's at a borderline score: a comparison of the duals is well-posed in all three routes only
    without such rows.  The float64 routes, whose screen sets are the oracle's, run a second time with rows bounded at 0: that is
    what takes solve_zero's bounded least squares on an unscreened wide group beyond its trivial case."""
    from util import make_gaussian

    dtype = np.float32 if route == "naive32" else np.float64
    f32 = dtype == np.float32
    d = make_gaussian(300, int(SIZES.sum()), seed=3, sparsity=0.5, dtype=dtype)
    X, y, n = d["X"], d["y"], 300
    # (295 columns on 300 rows: the path stops at 0.2 lmda_max, before the active columns come close to the rows and the Gram
    # matrix to singular, where no route reproduces another to 1e-6)
    kw = dict(groups=GROUPS, alpha=0.8, lmda_path_size=8, min_ratio=0.2, early_exit=False, tol=1e-7 if f32 else 1e-10,
              progress_bar=False)
    if f32:
        kw["newton_tol"] = 1e-5  # (test_constraint.py:676)
    if route == "cov64":
        Xc, yc = X - X.mean(axis=0), y - y.mean()
        A, v = np.asfortranarray(Xc.T @ Xc / n), Xc.T @ yc / n
        fit = lambda dense: ad.gaussian_cov(dense(A), v, constraints=_path_constraints(dtype, zero_rows), **kw)
        dev_m, ref_m = (lambda M: ad.matrix.dense(M, method="cov")), oracle.cov_dense
    else:
        fit = lambda dense: ad.grpnet(dense(X), ad.glm.gaussian(y, dtype=dtype), constraints=_path_constraints(dtype, zero_rows), **kw)
        dev_m, ref_m = ad.matrix.dense, oracle.dense
    ref = fit(ref_m)
    assert ref.error == "" and len(ref.lmdas) == 8
    # the problem exercises what it is here for: a wide group with non-zero coefficients held against a bound
    dg, Rd, Rb = np.asarray(ref.dual_groups), ref.duals.toarray(), ref.betas.toarray()
    assert any(np.any((Rd[:, dg[g]:dg[g] + m] != 0).any(axis=1) & (Rb[:, GROUPS[g]:GROUPS[g] + s] != 0).any(axis=1))
               for g, (m, s) in enumerate(zip(ROWS, SIZES)))
    st = fit(dev_m)
    assert st.error == "" and len(st.lmdas) == len(ref.lmdas)
    assert st.counters["n_host_cons_visits"] == 0 and st.counters["n_dev_cons_visits"] > 0, st.counters
    tol = 2e-3 if f32 else 1e-6  # (the tolerances of test_gpu_cons_linear.py's path test)
    B = st.betas.toarray()
    assert np.abs(B - Rb).max() < tol
    assert st.duals.shape == ref.duals.shape and ref.duals.nnz > 0
    dscale = max(1.0, float(np.abs(ref.duals).max()))
    assert np.abs((st.duals - ref.duals)).max() < (2e-2 * dscale if f32 else 1e-5)
    assert np.abs(st.abs_grad - ref.abs_grad).max() < (1e-2 if f32 else 1e-6)  # (solve_zero on the unscreened groups)
    os.environ["ADELIE_HIP_CONS_HOST"] = "1"
    try:
        sth = fit(dev_m)
    finally:
        del os.environ["ADELIE_HIP_CONS_HOST"]
    assert sth.error == "" and sth.counters["n_dev_cons_visits"] == 0 and sth.counters["n_host_cons_visits"] > 0
    assert np.abs(sth.betas.toarray() - B).max() < tol
    assert np.abs((sth.duals - st.duals)).max() < (2e-2 * dscale if f32 else 1e-5)
