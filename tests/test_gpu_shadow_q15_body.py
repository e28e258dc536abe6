"""The body loop of the 16-bit shadow sweep (shadow_sweep_kernel<ShadowQ15>, kernels_filter.hip), one launch at a time through
adelie_hip_filter_sweep_test with nothing listed (tstar = inf, no screen group): every value that comes back is the shadow's.

The loop runs the trips in which every lane has a 16-byte load as a rotation of two half panels, then a partial trip, then the
rows past the last whole load one at a time.  With w = 1 the swept vector is r itself, and for every column

    |shadow - fsum(xs_j o v)| <= fp_term nrm_j ||v||          (the body's own arithmetic against the copy it read)
    |shadow - fsum(x_j o v)|  <= (err_j + fp_term nrm_j) ||v||  (the bound the filter uses)

with xs_j = fl(scale_j q_j) the dequantised copy, err_j / nrm_j as the library measures them (test_shadow_kind_host), fp_term =
(4 n + 8) 2^-53 and both references summed exactly (test_shadow_fp_term.exact_dot; ||v|| = sqrt(fsum(v^2)), one rounding of 2^-53 against a bound
that is at least twice what the derivation in kernels_filter.hip needs)."""
import math
from fractions import Fraction

import numpy as np
import pytest

import adelie_amd as ad
from test_gpu_filter_sweep import fsweep
from test_shadow_fp_term import exact_dot
from test_shadow_kind_host import q15_encode, q15_err_nrm

pytestmark = pytest.mark.gpu

# rows: either side of the 8-row load and of the 2048 rows a workgroup takes per trip (0, 1 and 2 trips of the rotation: below
# 2048, from 2048, from 4096; 4097 adds a single row past the last load), 6145 for a second pass through the steady-state loop
ROWS = [1, 7, 8, 9, 2047, 2048, 2049, 4097, 6145]
COLS = [1, 7, 8, 9, 17]   # panel tails of the 8-column panel


def vectors(X, rng):
    n = X.shape[0]
    q, _ = q15_encode(X)
    mag = rng.uniform(0.5, 2.0, size=n)
    out = {"gaussian": rng.normal(size=n)}
    out["aligned with the last column"] = np.where(q[:, -1] >= 0, 1.0, -1.0) * mag
    out["aligned with the first column"] = np.where(q[:, 0] >= 0, 1.0, -1.0) * mag
    big = np.full(n, 1e-30) * np.where(rng.uniform(size=n) < 0.5, -1.0, 1.0)
    big[n // 2] = 1e30
    out["one row at 1e30 among rows at 1e-30"] = big
    ext = np.where(np.arange(n) % 2 == 0, 1e-40, 3e38) * np.where(rng.uniform(size=n) < 0.5, -1.0, 1.0)
    out["entries at 1e-40 and 3e38"] = ext
    out["zeros"] = np.zeros(n)
    return out


def check_body(monkeypatch, X):
    n, p = X.shape
    monkeypatch.setenv("ADELIE_HIP_SHADOW_KIND", "q15")
    monkeypatch.setenv("ADELIE_HIP_FILTER_SWEEP", "1")
    Xd = ad.matrix.dense(X)
    q, s = q15_encode(X)
    Xs = q * s                      # fl(scale q): one rounding per entry, as the copy is defined
    err, nrm = q15_err_nrm(X)
    fp_term = (4 * n + 8) * 2.0 ** -53
    groups = np.arange(p, dtype=np.int64)
    gsizes = np.ones(p, dtype=np.int64)
    pen = np.ones(p)
    w = np.ones(n)
    worst = 0.0
    for name, v in vectors(X, np.random.RandomState(n * 31 + p)).items():
        got, mask, info = fsweep(Xd, w, v, 0.0, None, [], groups, gsizes, pen, np.inf)
        assert info[2] == 1 and info[0] == 0 and info[1] == 0 and not mask.any(), (name, info)
        assert Xd.shadow_info()["kind"] == "q15"
        vnorm = math.sqrt(math.fsum(float(x) * float(x) for x in v))
        for j in range(p):
            xs_dot, x_dot = exact_dot(Xs[:, j], v), exact_dot(X[:, j], v)
            d_copy = abs(Fraction(float(got[j])) - xs_dot)
            d_true = abs(Fraction(float(got[j])) - x_dot)
            b_copy = Fraction(fp_term) * Fraction(float(nrm[j])) * Fraction(vnorm)
            b_true = (Fraction(float(err[j])) + Fraction(fp_term) * Fraction(float(nrm[j]))) * Fraction(vnorm)
            assert d_copy <= b_copy, (name, n, p, j, float(d_copy), float(b_copy))
            assert d_true <= b_true, (name, n, p, j, float(d_true), float(b_true))
            if b_copy > 0:
                worst = max(worst, float(d_copy / b_copy))
        if name == "zeros":
            assert not got.any()
    print("n = %d p = %d: largest |shadow - exact on the copy| / (fp_term nrm ||v||) = %.3g" % (n, p, worst))


@pytest.mark.parametrize("p", COLS)
@pytest.mark.parametrize("n", ROWS)
def test_q15_body_within_its_bound(hip, monkeypatch, n, p):
    X = np.asfortranarray(np.random.RandomState(1000 * p + n).normal(size=(n, p)))
    check_body(monkeypatch, X)


def test_q15_body_with_row_splits(hip, monkeypatch):
    """20000 x 24: three row splits of 8192, 8192 and 3616 rows (4, 4 and 1 whole trips, the last with a partial trip after it),
    their partials scaled and added by the reduce launch."""
    X = np.asfortranarray(np.random.RandomState(77).normal(size=(20000, 24)))
    check_body(monkeypatch, X)


def test_classification_matches_its_arithmetic_restated(hip, monkeypatch):
    """4000 x 300 in groups of 3, a tenth of the groups in the screen set, one group without a penalty: a group is listed when
    sqrt(sum g^2) + sqrt(sum b^2) ||v|| reaches tstar penalty on the shadow's values g, with b_j = err_j + fp_term nrm_j.  The
    shadow's values of a listed group are replaced by the exact ones before they come back, and |g_j - exact_j| <= b_j ||v||,
    so a listed group reaches the threshold with twice the bound on the exact values, an unlisted one stays below it on the
    values returned, and every listed group is listed whole."""
    from test_gpu_filter_sweep import make_problem
    monkeypatch.setenv("ADELIE_HIP_SHADOW_KIND", "q15")
    n, p, gs = 4000, 300, 3
    prob = make_problem(n, p, gs, seed=5)
    X, w, r, rsum, xm, groups, gsizes, pen = prob
    pen = pen.copy()
    pen[17] = 0.0
    screen = list(range(0, len(groups), 10))
    Xd = ad.matrix.dense(X)
    v = w * r
    exact = X.T @ v - rsum * xm
    norms = np.array([np.sqrt((exact[k:k + s] ** 2).sum()) for k, s in zip(groups, gsizes)])
    with np.errstate(divide="ignore"):
        tstar = np.quantile((norms / pen)[pen > 0], 0.85)
    monkeypatch.setenv("ADELIE_HIP_FILTER_SWEEP", "1")
    got, mask, info = fsweep(Xd, w, r, rsum, xm, screen, groups, gsizes, pen, tstar)
    assert info[2] == 1 and info[1] == 0 and info[0] > 0
    err, nrm = q15_err_nrm(X)
    b = err + (4 * n + 8) * 2.0 ** -53 * nrm
    vnorm = np.sqrt((v ** 2).sum()) * (1 + 1e-6)
    listed = 0
    for g, (k, s) in enumerate(zip(groups, gsizes)):
        cols = slice(k, k + s)
        if g in screen or pen[g] == 0:
            assert mask[cols].all()
            continue
        eps = np.sqrt((b[cols] ** 2).sum()) * vnorm
        assert mask[cols].all() or not mask[cols].any()
        if mask[cols].all():
            listed += s
            assert norms[g] + 2 * eps * (1 + 1e-6) >= tstar * pen[g]
        else:
            assert (np.sqrt((got[cols] ** 2).sum()) + eps) * (1 - 1e-9) < tstar * pen[g]
    assert listed == info[0] == info[3]
    monkeypatch.setenv("ADELIE_HIP_FILTER_SWEEP", "0")
    full, _, _ = fsweep(Xd, w, r, rsum, xm, screen, groups, gsizes, pen, tstar)
    assert got[mask].tobytes() == full[mask].tobytes()
