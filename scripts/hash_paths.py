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
