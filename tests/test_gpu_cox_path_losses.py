"""X.cox_path_losses (adelie_hip_design_cox_path_losses): the Cox losses of a path's etas under the full-data and the training
family, batched over lambda on the device.  Checked bit for bit against one adelie_hip_glm_cox_eval per eta and family (the
batched kernels run cox_eval's tiles and combination trees), against the numpy family with intercepts and offsets, on the other
design kinds, for its refusals, and as the route cv_grpnet takes for glm.cox."""
import functools

import numpy as np
import pytest
import scipy.sparse

import adelie_amd as ad
from test_cox import case
from test_gpu_cox import assert_close, big_case

pytestmark = pytest.mark.gpu

P = 6
SCALES = (0.0, 0.5, 1.0, 2.0, 3.0)   # row 0 is an empty CSR row (the first lambda of a path); max eta from 0 to about 12
L = len(SCALES)
SHAPES = [(n, ns, ties) for n in (1, 2, 1000, 3077) for ns in (1, 7, "pairs") for ties in (0, 10)]


@functools.lru_cache(maxsize=None)
def families(n, ns, ties, dtype):
    """The full-data family and the family of a training fold: a random fifth of the rows at weight zero."""
    fam, _ = big_case(n, ns, ties, seed=n % 97, dtype=dtype)
    wb = fam.weights * (np.random.default_rng(7).uniform(size=n) >= 0.2)
    if wb.sum() == 0:
        wb = fam.weights.copy()
    return fam, fam.reweight(wb / wb.sum())


@functools.lru_cache(maxsize=None)
def inputs(n, dtype):
    rng = np.random.default_rng(1000 + n)
    X = np.asfortranarray(rng.normal(0, 1, (n, P)), dtype=dtype)
    b = rng.normal(0, 1, P) / np.sqrt(P)
    betas = scipy.sparse.csr_matrix(np.outer(SCALES, b).astype(dtype))
    assert betas.indptr[1] == 0
    calls = np.asfortranarray(rng.integers(0, 3, (n, P)).astype(np.int8))
    mask = rng.uniform(size=(n, P)) < 0.3
    return X, betas, calls, mask


def make_design(kind, n, dtype):
    X, _, calls, mask = inputs(n, dtype)
    if kind == "dense":
        return ad.matrix.dense(X)
    if kind == "snp":
        return ad.matrix.snp_calldata(calls, dtype=dtype)
    if kind == "sparse":
        return ad.matrix.sparse(scipy.sparse.csc_matrix(X * mask), resident="csc")
    if kind == "pieces":   # two dense columns in front of a 2-bit block, each kept as it is
        return ad.matrix.concatenate([ad.matrix.dense(np.asfortranarray(X[:, :2])),
                                      ad.matrix.snp_calldata(np.asfortranarray(calls[:, 2:]), dtype=dtype)],
                                     axis=1, resident="pieces")
    if kind == "std":
        return ad.matrix.standardize(ad.matrix.snp_calldata(calls, dtype=dtype), lazy=True)
    raise ValueError(kind)


def device_etas(Xd, betas, n, dtype):
    etas = np.empty((L, n), dtype=dtype)
    Xd.sp_tmul(betas, etas)   # (a view composes its own: the base's product and the centring in numpy)
    return etas


def single_evals(fam, etas):
    return np.array([fam._device_eval(e, grad=False, hess=False)[2] for e in etas])


@functools.lru_cache(maxsize=None)
def dense_reference(n, ns, ties, dtype):
    """The design, its etas (downloaded) and one device evaluation per eta and family: computed once per shape."""
    fam, fb = families(n, ns, ties, dtype)
    Xd = make_design("dense", n, dtype)
    etas = device_etas(Xd, inputs(n, dtype)[1], n, dtype)
    ra, rb = single_evals(fam, etas), single_evals(fb, etas)
    for r in (etas, ra, rb):
        r.setflags(write=False)
    return Xd, etas, ra, rb


def check_bits(Xd, fam, fb, betas, ra, rb, max_batch):
    n = Xd.rows()
    zi, zo = np.zeros(L, dtype=Xd.dtype), np.zeros(n, dtype=Xd.dtype)
    for _ in range(2):   # the second call: no atomics, the same bits again
        a, b = Xd.cox_path_losses(fam, fb, betas, zi, zo, _max_batch=max_batch)
        assert a.dtype == b.dtype == np.float64 and a.shape == b.shape == (L,)
        print("full", a, ra, "train", b, rb)
        assert np.array_equal(a, ra)
        assert np.array_equal(b, rb)


@pytest.mark.parametrize("max_batch", [0, 2])   # 2: sub-batches of 2 + 2 + 1 etas
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n,ns,ties", SHAPES)
def test_bits_of_single_evaluations(hip, n, ns, ties, dtype, max_batch):
    """'pairs': strata whose training weights are all zero; ties: tie groups whose events all have zero training weight."""
    fam, fb = families(n, ns, ties, dtype)
    Xd, _, ra, rb = dense_reference(n, ns, ties, dtype)
    assert np.all(np.isfinite(ra)) and np.all(np.isfinite(rb))
    check_bits(Xd, fam, fb, inputs(n, dtype)[1], ra, rb, max_batch)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n,ns,ties", [s for s in SHAPES if s[0] >= 1000])
def test_against_numpy_family_with_intercepts_and_offsets(hip, n, ns, ties, dtype):
    fam, fb = families(n, ns, ties, dtype)
    Xd, etas, _, _ = dense_reference(n, ns, ties, dtype)
    rng = np.random.default_rng(3)
    b0 = rng.normal(0, 1, L).astype(dtype)
    off = (0.1 * rng.normal(0, 1, n)).astype(dtype)
    a, b = Xd.cox_path_losses(fam, fb, inputs(n, dtype)[1], b0, off)
    es = [(etas[l] + b0[l]) + off for l in range(L)]
    assert all(e.dtype == dtype for e in es)
    rtol = 1e-12 if dtype == np.float64 else 1e-5
    ra, rb = [float(fam.loss(e)) for e in es], [float(fb.loss(e)) for e in es]
    print("full", a, ra, "train", b, rb)
    assert_close(a, ra, rtol, 1.0)
    assert_close(b, rb, rtol, 1.0)


@pytest.mark.parametrize("kind", ["snp", "sparse", "std", "pieces"])
def test_other_design_kinds(hip, kind):
    n, ns, ties, dtype = 3077, 7, 10, np.float64
    fam, fb = families(n, ns, ties, dtype)
    Xd = make_design(kind, n, dtype)
    betas = inputs(n, dtype)[1]
    etas = device_etas(Xd, betas, n, dtype)
    ra, rb = single_evals(fam, etas), single_evals(fb, etas)
    assert np.ptp(ra) > 0
    for max_batch in (0, 2):
        check_bits(Xd, fam, fb, betas, ra, rb, max_batch)


def test_refusals(hip):
    n, dtype = 1000, np.float64
    fam, fb = families(n, 7, 10, dtype)
    Xd = make_design("dense", n, dtype)
    betas = inputs(n, dtype)[1]
    zi, zo = np.zeros(L), np.zeros(n)
    longer, _ = big_case(n + 1, 7, 10, seed=1, dtype=dtype)
    with pytest.raises(RuntimeError, match="cox_path_losses"):
        Xd.cox_path_losses(fam, longer, betas, zi, zo)
    f32, _ = big_case(n, 7, 10, seed=1, dtype=np.float32)
    with pytest.raises(RuntimeError, match="cox_path_losses"):
        Xd.cox_path_losses(f32, fb, betas, zi, zo)
    with pytest.raises(RuntimeError, match="cox_path_losses"):
        Xd.cox_path_losses(fam, ad.glm.gaussian(np.zeros(n)), betas, zi, zo)
    bad = scipy.sparse.csr_matrix(([1.0], [P - 1], [0, 0, 1, 1, 1, 1]), shape=(L, P))
    bad.indices[0] = P   # a column index past the design
    with pytest.raises(RuntimeError, match="cox_path_losses"):
        Xd.cox_path_losses(fam, fb, bad, zi, zo)


def test_cv_grpnet_takes_the_route(hip, monkeypatch):
    """The set-up of test_gpu_cox.test_cv_grpnet_cox.  With predict out of reach cv_grpnet still completes; its rows are the host
    route's (predict + glm.loss / glm_c.loss on the same fold solves, the last lines of cv._fold_loss restated) to the 1e-10 the
    existing test puts between two CV routes."""
    n, p = 600, 30
    start, stop, status, strata, w, _ = case(n, 81, n_strata=2, n_times=15)
    X = np.asfortranarray(np.random.default_rng(4).normal(0, 1, (n, p)))
    fam = ad.glm.cox(start, stop, status, strata=strata, weights=w)
    kw = dict(n_folds=4, lmda_path_size=15, seed=0, progress_bar=False)

    def no_predict(*a, **k):
        raise AssertionError("cv_grpnet left the device for a Cox fold's losses")

    with monkeypatch.context() as m:
        m.setattr(ad.cv, "predict", no_predict)
        r_seq = ad.cv_grpnet(ad.matrix.dense(X), fam, n_concurrent=1, **kw)
        r_def = ad.cv_grpnet(ad.matrix.dense(X), fam, **kw)
    assert np.all(np.isfinite(r_seq.losses)) and np.all(np.isfinite(r_def.losses))

    Xd = ad.matrix.dense(X)
    np.random.seed(0)
    order = np.random.choice(n, n, replace=False)
    ratios = np.logspace(0, np.log10(1e-1), 15)
    full_lmdas = ad.grpnet(Xd, fam, lmda_path_size=0, progress_bar=False).lmda_max * ratios
    np.testing.assert_array_equal(full_lmdas, r_seq.lmdas)
    for fold, (b, e) in enumerate(ad.cv.fold_ranges(n, 4)):
        idx = order[b:e]
        wt = fam.weights.copy()
        wt[idx] = 0
        wsum = np.sum(wt)
        fam_c = fam.reweight(wt / wsum)
        s0 = ad.grpnet(Xd, fam_c, lmda_path_size=0, progress_bar=False)
        curr = s0.lmda_max * ratios
        aug = np.sort(np.concatenate([full_lmdas, curr[curr > full_lmdas[0]]]))[::-1]
        s = ad.grpnet(Xd, fam_c, ddev_tol=0, early_exit=False, lmda_path=aug, progress_bar=False)
        fbeta, ficpt = ad.diagnostic.coefficients(lmdas_new=full_lmdas, betas=s.betas, intercepts=s.intercepts, lmdas=s.lmdas)
        etas = ad.diagnostic.predict(X=Xd, betas=fbeta, intercepts=ficpt, offsets=s._offsets)
        full = np.array([fam.loss(eta) for eta in etas])
        train = wsum * np.array([fam_c.loss(eta) for eta in etas])
        row = (full - train) / np.sum(fam.weights[idx])
        print(fold, r_seq.losses[fold], row)
        assert_close(r_seq.losses[fold], row, 1e-10, 1.0)
        assert_close(r_def.losses[fold], row, 1e-10, 1.0)
