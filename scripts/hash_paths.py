import os, sys, hashlib, numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import adelie_amd as ad
rng = np.random.RandomState(5)
n, p = 20037, 600
cd = np.asfortranarray(rng.choice([0, 1, 2, -9], size=(n, p), p=[0.6, 0.25, 0.05, 0.1]).astype(np.int8))
imp = np.array([cd[:, j][cd[:, j] >= 0].mean() for j in range(p)])
Xv = np.where(cd < 0, imp[None, :], cd).astype(float)
beta = np.zeros(p); beta[rng.choice(p, 200, replace=False)] = rng.normal(size=200) * 0.5
eta = Xv @ beta; eta = (eta - eta.mean()) / eta.std()
y = (rng.uniform(size=n) < 1 / (1 + np.exp(-2 * eta))).astype(float)
yg = eta + 0.3 * rng.normal(size=n)
X = ad.matrix.snp_calldata(cd, imp)
def digest(st, min_values=0, group_size=1):  # min_values: the leg must reach the block engines (screen sets of at least 128 values)
    assert st.error == "", st.error
    assert np.max(st.screen_sizes) * group_size >= min_values, np.max(st.screen_sizes)  # (screen_sizes counts groups)
    return hashlib.sha1(st.betas.toarray().tobytes()).hexdigest()[:16]
for name, glm, kw in [("binomial", ad.glm.binomial(y), dict(min_ratio=0.03, lmda_path_size=14)),
                      ("gaussian", ad.glm.gaussian(yg), dict(min_ratio=0.01, lmda_path_size=20))]:
    st = ad.grpnet(X, glm, early_exit=False, progress_bar=False, **kw)
    h = hashlib.sha1(st.betas.toarray().tobytes() + st.intercepts.tobytes()).hexdigest()[:16]
    print(name, h, st.counters["n_panel_blocks"], st.error)
kw_d = dict(early_exit=False, progress_bar=False, min_ratio=0.05, lmda_path_size=15)
Xd_h = np.asfortranarray(rng.normal(size=(3000, 900)))
Xd = ad.matrix.dense(Xd_h)
yd = rng.normal(size=3000)
st = ad.grpnet(Xd, ad.glm.gaussian(yd), **kw_d)
print("dense", digest(st), st.counters["n_panel_blocks"])
Xg_h = np.asfortranarray(rng.normal(size=(4000, 1200)))
Xg = ad.matrix.dense(Xg_h)
yg2 = rng.normal(size=4000)
st = ad.grpnet(Xg, ad.glm.gaussian(yg2), groups=np.arange(0, 1200, 10), alpha=0.5, **kw_d)
print("groups10", digest(st), st.counters["n_panel_blocks"])
Ym = rng.normal(size=(4000, 3))
st = ad.grpnet(Xg, ad.glm.multigaussian(Ym), early_exit=False, progress_bar=False, min_ratio=0.2, lmda_path_size=12)
print("multi3", digest(st), st.counters["n_panel_blocks"])
# the dense lasso again in single precision
st = ad.grpnet(ad.matrix.dense(np.asfortranarray(Xd_h.astype(np.float32))), ad.glm.gaussian(yd.astype(np.float32), dtype=np.float32), **kw_d)
print("dense_f32", digest(st), st.counters["n_panel_blocks"])
# ... and with a box on every coefficient: the panel engine's constrained solve (blk_solve_cons_kernel); last column: largest screen set
box = [ad.constraint.box(np.array([-0.02 * (j % 3)]), np.array([0.03])) for j in range(900)]
st = ad.grpnet(Xd, ad.glm.gaussian(yd), constraints=box, **kw_d)
print("dense_box", digest(st, 128), st.counters["n_panel_blocks"], int(np.max(st.screen_sizes)))
# covariance method, the full-Gram engines: lasso (blk_solve_kernel) and groups of 10 (grp_solve_kernel's full-Gram form)
def cov_of(Xh, yh):
    Xc = Xh - Xh.mean(axis=0)
    return np.asfortranarray(Xc.T @ Xc / len(yh)), Xc.T @ (yh - yh.mean()) / len(yh)
A, v = cov_of(Xd_h, yd)
st = ad.gaussian_cov(A=A, v=v, **kw_d)
print("cov_lasso", digest(st, 128), st.counters["n_panel_blocks"], int(np.max(st.screen_sizes)))
A, v = cov_of(Xg_h, yg2)
st = ad.gaussian_cov(A=A, v=v, groups=np.arange(0, 1200, 10), alpha=0.5, **kw_d)
print("cov_groups10", digest(st, 128, 10), st.counters["n_panel_blocks"], int(np.max(st.screen_sizes)))
# the storage kinds the legs above do not reach: compressed columns (Gaussian, binomial), lazily standardized views of the dense
# and of the 2-bit design (alpha = 0.5: the views' own engines, the std-view branches of sweep / gram / axpy_cols), one_hot
import scipy.sparse as sp
Xs_h = sp.random(3000, 400, density=0.05, random_state=rng, format="csc", dtype=np.float64)
Xs = ad.matrix.sparse(Xs_h, resident="csc")
ys = np.asarray(Xs_h @ (rng.normal(size=400) * (rng.uniform(size=400) < 0.1))).ravel() + 0.3 * rng.normal(size=3000)
st = ad.grpnet(Xs, ad.glm.gaussian(ys), **kw_d)
print("csc_gaussian", digest(st), st.counters["n_panel_blocks"])
st = ad.grpnet(Xs, ad.glm.binomial((ys > np.median(ys)).astype(float)), early_exit=False, progress_bar=False, min_ratio=0.1,
               lmda_path_size=12)
print("csc_binomial", digest(st), st.counters["n_panel_blocks"])
st = ad.grpnet(ad.matrix.standardize(Xd, lazy=True), ad.glm.gaussian(yd), alpha=0.5, **kw_d)
print("std_dense_a05", digest(st), st.counters["n_panel_blocks"])
st = ad.grpnet(ad.matrix.standardize(X, lazy=True), ad.glm.gaussian(yg), alpha=0.5, early_exit=False, progress_bar=False,
               min_ratio=0.05, lmda_path_size=12)
print("std_snp_a05", digest(st), st.counters["n_panel_blocks"])
Zt = np.asfortranarray(np.stack([rng.randint(0, 5, size=3000), rng.normal(size=3000), rng.randint(0, 40, size=3000)], axis=1).astype(float))
Xo = ad.matrix.one_hot(Zt, np.array([5, 0, 40]))
st = ad.grpnet(Xo, ad.glm.gaussian(yd), groups=Xo.groups, **kw_d)
print("one_hot", digest(st), st.counters["n_panel_blocks"], st.counters["n_sweeps_factor"])
# the matrix operations per storage kind: one digest over the result bytes of every raw operation (lazy_cov: dense and 2-bit only)
def ops_digest(M, with_cov):
    r = np.random.RandomState(9)
    n_, p_ = M.shape
    dt = M.dtype
    f = lambda a: np.asarray(a, dtype=dt)
    v, w, sw = f(r.normal(size=n_)), f(r.uniform(0.5, 1.5, size=n_)), f(r.uniform(0.5, 1.5, size=n_))
    h = hashlib.sha1()
    o = np.empty(p_, dtype=dt); M.mul(v, w, o); h.update(o.tobytes())
    o = np.empty(9, dtype=dt); M.bmul(5, 9, v, w, o); h.update(o.tobytes())
    o = f(r.normal(size=n_)); M.btmul(5, 9, f(r.normal(size=9)), o); h.update(o.tobytes())
    o = np.empty((9, 9), dtype=dt); M.cov(5, 9, sw, o); h.update(np.ascontiguousarray(o).tobytes())
    o = np.empty(p_, dtype=dt); M.sq_mul(w, o); h.update(o.tobytes())
    B = sp.random(4, p_, density=0.2, random_state=r, format="csr", dtype=np.float64)
    o = np.empty((4, n_), dtype=dt); M.sp_tmul(B.astype(dt), o); h.update(o.tobytes())
    h.update(M.mul_batch(f(r.normal(size=(9, n_)))).tobytes())
    wa = r.uniform(0.5, 1.5, size=n_); wa /= wa.sum()
    wb = wa * (r.uniform(size=n_) < 0.8); wb /= wb.sum()
    for part in M.glm_path_losses(1, B, r.normal(size=4), 0.1 * r.normal(size=n_), (r.uniform(size=n_) < 0.4).astype(float), wa, wb):
        h.update(np.asarray(part).tobytes())
    BK = sp.random(4, p_ * 3, density=0.1, random_state=r, format="csr", dtype=np.float64)
    for part in M.multi_path_losses(0, 3, BK, r.normal(size=(4, 3)), 0.1 * r.normal(size=(n_, 3)), r.normal(size=(n_, 3)), wa, wb):
        h.update(np.asarray(part).tobytes())
    if with_cov:
        A = ad.matrix.lazy_cov(M)
        o = np.empty((p_, p_), dtype=dt); A.to_dense(0, p_, o); h.update(np.ascontiguousarray(o).tobytes())
    return h.hexdigest()[:16]
Xo_h = np.asfortranarray(rng.normal(size=(2003, 300)))
Mo = ad.matrix.dense(Xo_h)
# (handles that borrow their arrays -- an alias, a column slice -- and the derived 2-bit, convex-relu and phased designs included)
rmask = np.random.RandomState(12).uniform(size=(2003, 4)) < 0.5
Zs_h = sp.random(2003, 10, density=0.2, random_state=np.random.RandomState(13), format="csc", dtype=np.float64)
pr = np.random.RandomState(14)
for name, M, with_cov in [("dense_f64", Mo, True),
                          ("dense_f32", ad.matrix.dense(np.asfortranarray(Xo_h.astype(np.float32))), True),
                          ("snp", X, True), ("csc", Xs, False), ("std_csc", ad.matrix.standardize(Xs), False),
                          ("alias_dense", Mo.alias(), True), ("slice_dense", ad.matrix.subset(Mo, np.arange(10, 110), axis=1), True),
                          ("concat_snp", ad.matrix.concatenate([X, X], axis=1), True),
                          ("subset_snp", ad.matrix.subset(X, np.arange(0, 600, 3), axis=1), True),
                          ("relu_dense", ad.matrix.convex_relu(Xo_h[:, :6], rmask), True),
                          ("relu_csc", ad.matrix.convex_relu(Zs_h, rmask, resident="csc"), False),
                          ("phased", ad.matrix.snp_phased_calldata(pr.randint(0, 2, size=(2003, 40)).astype(np.int8),
                                                                   pr.randint(0, 3, size=(2003, 40)).astype(np.int8), 3), False)]:
    print("ops", name, ops_digest(M, with_cov))
# the filtered invariance sweep at kernel level, per shadow kind: grad (the shadow's own values in the unlisted columns included),
# the exact mask and info of adelie_hip_filter_sweep_test, with screen groups and one group without a penalty
def filter_digest(n, p, gs, intercept, kind):
    os.environ["ADELIE_HIP_SHADOW_KIND"] = kind
    os.environ["ADELIE_HIP_FILTER_SWEEP"] = "1"
    r_ = np.random.RandomState(n + p + gs)
    Xh = np.asfortranarray(r_.normal(size=(n, p)))
    w = r_.uniform(0.5, 1.5, size=n); w[::3] = 0.0; w /= w.sum()
    r = r_.normal(size=n)
    groups = np.arange(0, p, gs, dtype=np.int64)
    gsizes = np.minimum(gs, p - groups).astype(np.int64)
    pen = r_.uniform(0.5, 2.0, size=len(groups)); pen[2] = 0.0
    xm = (Xh.T @ w) if intercept else None
    rsum = float((w * r).sum()) if intercept else 0.0
    g0 = Xh.T @ (w * r) - (rsum * xm if intercept else 0.0)
    score = np.array([np.sqrt((g0[k:k + s] ** 2).sum()) for k, s in zip(groups, gsizes)]) / np.where(pen > 0, pen, np.inf)
    screen = np.arange(0, len(groups), 7, dtype=np.int64)
    M = ad.matrix.dense(Xh)
    grad, exact, info = np.empty(p), np.zeros(p, dtype=np.uint8), np.zeros(4, dtype=np.int64)
    ptr = lambda a: a.ctypes.data if a is not None else None
    b = M._backend
    b.check(b.fn("filter_sweep_test")(M._handle, ptr(w), ptr(r), rsum, ptr(xm), ptr(screen), len(screen), ptr(groups), ptr(gsizes),
                                      len(groups), ptr(pen), float(np.quantile(score, 0.9)), ptr(grad), ptr(exact), ptr(info)))
    assert info[2] == 1 and 0 < exact.sum() < p, (info, exact.sum())   # routed through the filter, shadow values left in grad
    return hashlib.sha1(grad.tobytes() + exact.tobytes() + info.tobytes()).hexdigest()[:16], int(exact.sum()), info.tolist()
saved_env = {k: os.environ.get(k) for k in ("ADELIE_HIP_SHADOW_KIND", "ADELIE_HIP_FILTER_SWEEP")}   # (the caller's, put back below)
for kind in ("f32", "q15"):
    for n_, p_, gs, icpt in [(5000, 37, 4, False), (1000, 4100, 1, True), (5003, 37, 1, True), (20000, 24, 1, True)]:
        print("filter", kind, (n_, p_), *filter_digest(n_, p_, gs, icpt, kind))
for k, val in saved_env.items():
    if val is None:
        os.environ.pop(k, None)
    else:
        os.environ[k] = val
# solver.bvls and solver.pinball (cd_screen_driver.hpp, state._ScreenSetState) on the inputs of the tests' restatements: one
# digest per leg over beta, resid, grad, the ordered sets, the flags, loss, iters, n_kkt and error (pinball: screen_AS and
# screen_ASAT_diag as well); after it ns, iters, n_kkt
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import bvls_checks as bc, pinball_checks as pc
def cd_digest(st):
    h = hashlib.sha1()
    for a in (st.beta, st.resid, st.grad, st.screen_set[:st.screen_set_size], st.active_set[:st.active_set_size], st.is_screen, st.is_active):
        h.update(np.ascontiguousarray(a).tobytes())
    h.update(repr((st.loss, st.iters, st.n_kkt, st.error)).encode())
    if hasattr(st, "screen_AS"):
        h.update(np.ascontiguousarray(st.screen_AS).tobytes() + st.screen_ASAT_diag.tobytes())
    return h.hexdigest()[:16], int(st.screen_set_size), st.iters, st.n_kkt
def with_config(name, value, default, solve):
    b = ad._abi.hip_backend()
    b.check(b.fn("set_config")(name.encode(), float(value)))
    try:
        return solve()
    finally:
        b.check(b.fn("set_config")(name.encode(), float(default)))
def cd_legs(name, solve, small, crossing):
    """`small` ends by the KKT pass; `crossing` is solved with kappa = 7 and passes ns = 64 (the resident matrix is regrown with
    members in it)."""
    cold = solve(small)
    assert cold.error == "", cold.error
    print(name, "cold", *cd_digest(cold))
    k7 = solve(crossing, kappa=7)
    assert k7.error == "" and k7.screen_set_size > 64 and k7.n_kkt > 10, (k7.error, k7.screen_set_size)
    print(name, "kappa7", *cd_digest(k7))
    print(name, "warm", *cd_digest(solve(small, tol=1e-9, warm_start=cold)))
    print(name, "global", *cd_digest(with_config(name.split()[0] + "_lds_max_ns", 16, 0, lambda: solve(crossing, kappa=7))))
    st = solve(crossing, max_iters=3)
    assert st.error.endswith("max iterations reached!"), st.error
    print(name, "max_iters", *cd_digest(st))
    st = with_config(name.split()[0] + "_gram_limit_mb", 0.0005, 16384, lambda: solve(crossing, kappa=7))   # 524 bytes: 7 x 7 fit, 14 x 14 do not
    assert "screen set of 14 coordinates" in st.error and st.screen_set_size == 7, st.error
    print(name, "gram_limit", *cd_digest(st))
for dt in (np.float64, np.float32):
    def bvls_solve(case, **kw):
        Xb, yb, lo, up = bc.gaussian(*case)
        return ad.bvls(np.asfortranarray(Xb, dtype=dt), yb.astype(dt), lo, up, **kw)
    cd_legs("bvls " + np.dtype(dt).name, bvls_solve, (200, 70, 0), (64, 300, 0))
    st = bvls_solve((400, 2000, 0), kappa=2000)
    assert st.error == "" and st.screen_set_size > 1024, (st.error, st.screen_set_size)
    print("bvls", np.dtype(dt).name, "ns>1024", *cd_digest(st))
    def pinball_solve(case, **kw):
        Ap, Sp, vp, pneg, ppos = pc.gen(*case)
        return ad.pinball(Ap.astype(dt), np.asfortranarray(Sp.astype(dt)), vp.astype(dt), pneg, ppos, **kw)
    cd_legs("pinball " + np.dtype(dt).name, pinball_solve, (130, 40, 0, 0.3), (300, 64, 0, 0.1))
# the routes through the matrix interface: bvls on a lazily standardized design, pinball with the resident matrix routed there
Xb, yb, lo, up = bc.gaussian(40, 13, 0)
st = ad.bvls(ad.matrix.standardize(ad.matrix.dense(Xb), lazy=True), yb, lo, up)
assert st.error == "" and not hasattr(st, "benchmark")
print("bvls python_route", *cd_digest(st))
native_rule, ad.state._pinball_native = ad.state._pinball_native, lambda A: False
try:
    st = ad.pinball(*pc.gen(20, 5, 0, 1.0))
finally:
    ad.state._pinball_native = native_rule
assert st.error == "" and st.benchmark.keys() == {"n_changed"}
print("pinball python_route", *cd_digest(st), st.benchmark["n_changed"])
