"""glm.cox, the numpy family: against a brute-force O(n^2) restatement of the documented loss, finite differences,
invariances, argument handling and the survival sampler of data.dense.  No GPU."""
import numpy as np
import pytest

import adelie_amd as ad


def brute(start, stop, status, strata, weights, tie_method, eta):
    """loss, -d loss / d eta, and the diagonal of d^2 loss / d eta^2 from the definition (reference glm.py:211-289):
    R(u) = {k : s_k < u <= t_k} inside the stratum, H(u) = events at u with non-zero weight, wbar their mean weight, sigma the
    Efron scale k / |H| (k the rank among H, in row order) or 0 (Breslow)."""
    n = len(stop)
    eta = np.asarray(eta, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64)
    d = np.asarray(status, dtype=np.float64)
    z = w * np.exp(eta)
    same = strata[:, None] == strata[None, :]
    R = same & (start[None, :] < stop[:, None]) & (stop[:, None] <= stop[None, :])          # R[i, k]: k at risk at t_i
    ev = (d == 1) & (w != 0)
    H = same & (stop[:, None] == stop[None, :]) & ev[None, :] & ev[:, None]                  # H[i, k]: both events tied
    size = H.sum(axis=1)
    wbar = np.where(ev, (H * w[None, :]).sum(axis=1) / np.maximum(size, 1), 0.0)
    if tie_method == "efron":
        rank = np.array([np.sum(H[i, :i]) for i in range(n)])
        sigma = np.where(ev & (size > 0), rank / np.maximum(size, 1), 0.0)
    else:
        sigma = np.zeros(n)
    M = R - sigma[:, None] * H                                                            # (R - sigma H)[i, k]
    D = M @ z
    a = wbar * d
    with np.errstate(divide="ignore"):
        loss = -np.sum(w * d * eta) + np.sum(np.where(a != 0, a * np.log(np.where(a != 0, D, 1.0)), 0.0))
    inv = np.where(a != 0, a / np.where(a != 0, D, 1.0), 0.0)
    grad = w * d - z * (M.T @ inv)
    inv2 = np.where(a != 0, a / np.where(a != 0, D, 1.0) ** 2, 0.0)
    M2 = R - (sigma * (2 - sigma))[:, None] * H
    hess = (w * d - grad) - z * z * (M2.T @ inv2)
    with np.errstate(divide="ignore"):
        lf = np.where(a != 0, np.log(np.where(a != 0, size * wbar * (1 - sigma), 1.0)), 0.0)
    loss_full = np.sum(a * lf)
    return loss, grad, hess, loss_full


def family_eval(fam, eta):
    n = len(eta)
    g = np.empty(n)
    h = np.empty(n)
    fam.gradient(eta, g)
    fam.hessian(eta, g, h)
    return fam.loss(eta), g, h, fam.loss_full()


def case(n, seed, *, n_strata=1, n_times=None, trunc=True, zero_w=0.0, censor=0.3):
    rng = np.random.default_rng(seed)
    start = np.round(rng.exponential(1, n), 1) if trunc else np.zeros(n)
    dt = rng.integers(1, n_times + 1, n).astype(float) if n_times else np.round(rng.exponential(2, n), 1) + 0.1
    stop = start + dt
    if n_times:
        stop = np.floor(start) + dt  # ties in stop across rows with different starts
        start = np.minimum(start, stop - 0.05)
    status = (rng.uniform(size=n) > censor).astype(float)
    strata = rng.integers(0, n_strata, n)
    strata = np.unique(strata, return_inverse=True)[1]
    w = rng.uniform(0.5, 2, n) * (rng.uniform(size=n) >= zero_w)
    if w.sum() == 0:
        w[0] = 1
    eta = rng.normal(0, 1, n)
    return start, stop, status, strata, w, eta


def close(a, b, rtol, floor=1e-300):
    """max |a - b| <= rtol * max(max |b|, floor): relative to the output's scale (a gradient that cancels to ~0 at some rows is
    compared at the scale of its terms, `floor` = the largest weight)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = max(np.max(np.abs(b)) if b.size else 0.0, floor)
    assert np.max(np.abs(a - b)) <= rtol * scale, (np.max(np.abs(a - b)), scale)


CASES = [
    dict(n=1, seed=0),
    dict(n=2, seed=1),
    dict(n=40, seed=2),
    dict(n=60, seed=3, n_times=4),                        # heavy ties
    dict(n=60, seed=4, n_strata=5, n_times=6),            # strata
    dict(n=50, seed=5, zero_w=0.3, n_times=5),            # zero weights inside ties
    dict(n=50, seed=6, trunc=False, n_times=3),           # no truncation, giant ties
    dict(n=30, seed=7, n_strata=3, censor=0.8, n_times=3),  # censored rows inside event ties, sparse events
    dict(n=80, seed=8, n_strata=40, n_times=2),           # strata of ~2 rows
]


@pytest.mark.parametrize("tie_method", ["efron", "breslow"])
@pytest.mark.parametrize("c", CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_numpy_family_matches_brute_force(c, tie_method):
    start, stop, status, strata, w, eta = case(**c)
    fam = ad.glm.cox(start, stop, status, strata=strata, weights=w, tie_method=tie_method)
    got = family_eval(fam, eta)
    ref = brute(start, stop, status, strata, fam.weights, tie_method, eta)
    for a, b in zip(got, ref):
        close(a, b, 1e-12, fam.weights.max())


def test_all_censored_stratum():
    start, stop, status, strata, w, eta = case(40, 11, n_strata=2, n_times=4)
    status[strata == 1] = 0
    fam = ad.glm.cox(start, stop, status, strata=strata, weights=w)
    got = family_eval(fam, eta)
    ref = brute(start, stop, status, strata, fam.weights, "efron", eta)
    for a, b in zip(got, ref):
        close(a, b, 1e-12, fam.weights.max())
    # an all-censored stratum contributes nothing but its rows' (zero) gradient
    assert np.all(got[1][strata == 1] <= 0)


@pytest.mark.parametrize("tie_method", ["efron", "breslow"])
def test_gradient_and_hessian_are_derivatives(tie_method):
    """grad = -d loss / d eta and hess = diag(-d grad / d eta), by central differences.  The diagonal Hessian of the family is
    the exact diagonal for Efron too: with H(t_i) inside R(t_i), (R - sigma H)^2 = R - sigma (2 - sigma) H entrywise."""
    start, stop, status, strata, w, eta = case(30, 12, n_strata=2, n_times=4)
    fam = ad.glm.cox(start, stop, status, strata=strata, weights=w, tie_method=tie_method)
    _, g, h, _ = family_eval(fam, eta)
    eps = 1e-6
    for j in range(len(eta)):
        e = np.zeros(len(eta))
        e[j] = eps
        dl = (fam.loss(eta + e) - fam.loss(eta - e)) / (2 * eps)
        gp, gm = np.empty(len(eta)), np.empty(len(eta))
        fam.gradient(eta + e, gp)
        fam.gradient(eta - e, gm)
        dg = (gp[j] - gm[j]) / (2 * eps)
        assert abs(-dl - g[j]) <= 1e-7 * max(1, abs(g[j])), j
        assert abs(-dg - h[j]) <= 1e-6 * max(1e-3, abs(h[j])), j


def test_shift_and_permutation_invariance():
    start, stop, status, strata, w, eta = case(70, 13, n_strata=3, n_times=5)
    fam = ad.glm.cox(start, stop, status, strata=strata, weights=w)
    l0, g0, h0, _ = family_eval(fam, eta)
    l1, g1, h1, _ = family_eval(fam, eta + 7.5)
    wm = fam.weights.max()
    close(l1, l0, 1e-12, wm)
    close(g1, g0, 1e-12, wm)
    close(h1, h0, 1e-12, wm)
    perm = np.random.default_rng(0).permutation(len(eta))
    famp = ad.glm.cox(start[perm], stop[perm], status[perm], strata=strata[perm], weights=w[perm])
    lp, gp, hp, lfp = family_eval(famp, eta[perm])
    close(lp, l0, 1e-12, wm)
    close(gp, g0[perm], 1e-12, wm)
    close(hp, h0[perm], 1e-12, wm)


def test_breslow_ignores_row_order_inside_ties_efron_sums_do_not_change():
    # rows of one tie group reordered: Breslow outputs permute exactly; Efron's per-row scales move with the rows but the
    # loss does not change (the scales of a tie are a fixed set)
    start = np.zeros(6)
    stop = np.array([1.0, 2, 2, 2, 3, 3])
    status = np.array([1.0, 1, 1, 0, 1, 1])
    eta = np.array([0.1, -0.3, 0.5, 0.2, 0.0, 0.4])
    perm = np.array([0, 3, 2, 1, 5, 4])
    for tm in ("efron", "breslow"):
        f0 = ad.glm.cox(start, stop, status, tie_method=tm)
        f1 = ad.glm.cox(start[perm], stop[perm], status[perm], tie_method=tm)
        close(f1.loss(eta[perm]), f0.loss(eta), 1e-12, 1.0)
        if tm == "breslow":
            g0, g1 = np.empty(6), np.empty(6)
            f0.gradient(eta, g0)
            f1.gradient(eta[perm], g1)
            close(g1, g0[perm], 1e-12, 1.0)


def test_arguments_dtype_and_reweight():
    start, stop, status, strata, w, eta = case(20, 14, n_strata=2, n_times=3)
    fam = ad.glm.cox(start, stop, status, strata=strata, weights=w)
    assert fam.name == "cox" and fam.is_multi is False and fam.core_kind == ad._abi.GLM_COX
    assert fam.tie_method == "efron"
    assert fam.dtype == np.float64 and fam.y is fam.status
    assert np.isclose(fam.weights.sum(), 1)
    f32 = ad.glm.cox(start, stop, status.astype(np.float32))
    assert f32.dtype == np.float32 and f32.weights.dtype == np.float32 and isinstance(f32, ad.glm.GlmBase32)
    assert np.all(ad.glm.cox(start, stop, status).strata == 0)
    with pytest.raises(RuntimeError, match="y must have an underlying type"):
        ad.glm.cox(start, stop, status.astype(int))
    with pytest.raises(RuntimeError, match="start must be"):
        ad.glm.cox(start[:-1], stop, status)
    with pytest.raises(RuntimeError, match="stop must be"):
        ad.glm.cox(start, stop[:-1], status)
    with pytest.raises(RuntimeError, match="strata must be"):
        ad.glm.cox(start, stop, status, strata=strata[:-1])
    with pytest.raises(RuntimeError, match="Invalid tie method"):
        ad.glm.cox(start, stop, status, tie_method="exact")
    with pytest.raises(RuntimeError, match="y and weights"):
        ad.glm.cox(start, stop, status, weights=w[:-1])
    w2 = np.arange(1, 21, dtype=float)
    r = fam.reweight(w2)
    assert r.name == "cox" and r.tie_method == fam.tie_method
    assert np.array_equal(r.start, fam.start) and np.array_equal(r.stop, fam.stop) and np.array_equal(r.strata, fam.strata)
    assert np.allclose(r.weights, w2 / w2.sum())
    assert r._orders is fam._orders  # the sort orders are shared, not recomputed
    ref = ad.glm.cox(start, stop, status, strata=strata, weights=w2)
    close(r.loss(eta), ref.loss(eta), 1e-14, 1.0)
    out = np.empty(20)
    r.inv_link(eta, out)
    assert np.allclose(out, np.exp(eta))


def test_data_dense_cox():
    d = ad.data.dense(200, 30, 30, glm="cox", seed=3)
    g = d["glm"]
    assert g.name == "cox" and d["X"].shape == (200, 30)
    assert g.start.shape == g.stop.shape == g.status.shape == (200,)
    assert np.all(g.start >= 0) and np.all(g.stop > g.start)
    assert set(np.unique(g.status)) <= {0.0, 1.0}
    assert 0 < g.status.sum() < 200
