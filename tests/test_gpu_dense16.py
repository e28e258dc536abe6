"""matrix.dense on float16 / bfloat16 input: a design kept 16-bit in HBM (kernels_dense16.hip), against float64 numpy on the
stored values.  Every stored value is exactly a float32 value, so the yardstick is the float32 dense design of the same values:
the 16-bit design's error against float64 may be at most 4 times that design's, plus n * eps32 * max|terms| (the rounding of
an n-term float32 sum), entry by entry."""
import numpy as np
import pytest
from scipy.sparse import csr_matrix

import adelie_amd as ad

pytestmark = pytest.mark.gpu
EPS32 = float(np.finfo(np.float32).eps)

# (n, p, sliced): the issue's shapes; (16, 5, sliced) has a base pointer 2 bytes off a 16-byte boundary; (2100, 3) crosses the
# sweep's 2048-row tile, (8300, 3) its row splits, (300, 70) the Gram's 64-column tile
SHAPES = [(1, 1, False), (7, 3, False), (8, 2, False), (9, 5, False), (65, 17, False), (257, 33, False), (16, 5, True),
          (2100, 3, False), (8300, 3, False), (300, 70, False)]
CASES = [(f, o, s) for f in ("f16np", "f16", "bf16") for o in "FC" for s in SHAPES if not (f == "f16np" and s[2])]


def _case(fmt, order, n, p, sliced, seed=0):
    """The values (float32, exactly representable in the format) and the 16-bit design made from them."""
    import torch

    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, p)).astype(np.float32)
    if fmt == "bf16":
        X = (X.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
        special = list((np.array([1e30, -0.0], np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32))
    else:
        X = X.astype(np.float16).astype(np.float32)
        special = [np.float32(65504.0), np.float32(2.0 ** -24), np.float32(-0.0)]
    flat = X.reshape(-1)
    flat[:min(len(special), flat.size)] = special[:flat.size]  # (row 0: the special values stand in the first columns)
    if fmt == "f16np":
        return X, ad.matrix.dense(np.array(X.astype(np.float16), order=order))
    tdt = torch.bfloat16 if fmt == "bf16" else torch.float16
    src = torch.from_numpy(np.ascontiguousarray(X if order == "C" else X.T)).to("cuda").to(tdt)
    buf = torch.empty(n * p + 1, dtype=tdt, device="cuda")
    flat_t = buf[1:] if sliced else buf[:n * p]
    flat_t.copy_(src.reshape(-1))
    t = flat_t.view(n, p) if order == "C" else flat_t.view(p, n).t()
    assert not sliced or t.data_ptr() % 16 == 2
    return X, ad.matrix.dense(t)


def _check(name, got16, got32, ref, floor):
    with np.errstate(invalid="ignore", over="ignore"):
        e16, e32 = np.abs(np.asarray(got16, float) - ref), np.abs(np.asarray(got32, float) - ref)
        fin = np.isfinite(ref) & np.isfinite(floor) & np.isfinite(got32)  # (the last assertion holds the rest to the same)
        print(f"  {name}: max err 16-bit {np.max(e16[fin], initial=0):.3e} float32 dense {np.max(e32[fin], initial=0):.3e}")
        assert np.all(e16[fin] <= 4 * e32[fin] + floor[fin]), name
        assert np.array_equal(np.isfinite(got16), np.isfinite(got32)), name  # (beyond float32 in both, or in neither)


@pytest.mark.filterwarnings("ignore:Detected matrix to be C-contiguous")
@pytest.mark.parametrize("fmt,order,shape", CASES, ids=lambda c: str(c).replace(" ", ""))
def test_matrix_operations_against_float64(hip, fmt, order, shape):
    n, p, sliced = shape
    X, D = _case(fmt, order, n, p, sliced)
    R = ad.matrix.dense(np.asfortranarray(X))  # the float32 dense design of the same values
    assert D._kind == "dense16" and D.dtype == np.float32 and D.shape == (n, p) and (D.rows(), D.cols()) == (n, p)
    X64 = X.astype(np.float64)
    rng = np.random.default_rng(1)
    v = rng.normal(size=n).astype(np.float32)
    w = rng.uniform(0.5, 1.5, size=n).astype(np.float32)
    vw = v.astype(np.float64) * w
    j = 1 if p > 1 else 0
    q = p - j
    A64 = np.abs(X64)

    def both(fn):
        a, b, c = fn(D), fn(D), fn(R)
        assert np.array_equal(a, b, equal_nan=True), "two calls differ"
        return a, c

    def mul(M):
        out = np.empty(p, np.float32)
        M.mul(v, w, out)
        return out
    _check("mul", *both(mul), vw @ X64, n * EPS32 * (A64 * np.abs(vw)[:, None]).max(axis=0))

    def bmul(M):
        out = np.empty(q, np.float32)
        M.bmul(j, q, v, w, out)
        return out
    _check("bmul", *both(bmul), vw @ X64[:, j:], n * EPS32 * (A64[:, j:] * np.abs(vw)[:, None]).max(axis=0))

    coef = rng.normal(size=p).astype(np.float32)
    out0 = rng.normal(size=n).astype(np.float32)

    def btmul(M):
        out = out0.copy()
        M.btmul(0, p, coef, out)
        return out
    terms = np.maximum((A64 * np.abs(coef.astype(np.float64))[None]).max(axis=1), np.abs(out0))
    _check("btmul", *both(btmul), out0 + X64 @ coef.astype(np.float64), max(n, p + 1) * EPS32 * terms)

    sw = np.sqrt(w)

    def cov(M):
        out = np.empty((q, q), np.float32, order="F")
        M.cov(j, q, sw, out)
        return np.array(out)
    w64 = sw.astype(np.float64) ** 2
    Xq = X64[:, j:]
    with np.errstate(over="ignore", invalid="ignore"):
        tmax = np.max(np.abs(Xq)[:, :, None] * np.abs(Xq)[:, None, :] * w64[:, None, None], axis=0)
        _check("cov", *both(cov), (Xq * w64[:, None]).T @ Xq, (n + 1) * EPS32 * tmax)

        def sq_mul(M):
            out = np.empty(p, np.float32)
            M.sq_mul(w, out)
            return out
        sq_ref, sq_floor = w.astype(np.float64) @ X64 ** 2, n * EPS32 * (X64 ** 2 * w[:, None]).max(axis=0)
        _check("sq_mul", *both(sq_mul), sq_ref, sq_floor)

        def mean(M):
            out = np.empty(p, np.float32)
            M.mean(w, out)
            return out
        m_ref = w.astype(np.float64) @ X64
        _check("mean", *both(mean), m_ref, n * EPS32 * (A64 * w[:, None]).max(axis=0))

        cen = rng.normal(size=p).astype(np.float32)
        c64, sum_w = cen.astype(np.float64), float(np.sum(w.astype(np.float64)))

        def var(M):
            out = np.empty(p, np.float32)
            M.var(cen, w, out)
            return out
        v_floor = sq_floor + 4 * EPS32 * (np.abs(sq_ref) + np.abs(c64) * (np.abs(c64) * sum_w + 2 * np.abs(m_ref)))
        _check("var", *both(var), sq_ref + c64 * (c64 * sum_w - 2 * m_ref), v_floor + n * EPS32 * np.abs(c64) * (A64 * w[:, None]).max(axis=0) * 2)

    V = csr_matrix(np.where(rng.uniform(size=(3, p)) < 0.6, rng.normal(size=(3, p)), 0).astype(np.float32))

    def sp_tmul(M):
        out = np.empty((3, n), np.float32)
        M.sp_tmul(V, out)
        return out
    Vd = V.toarray().astype(np.float64)
    sp_floor = max(n, p) * EPS32 * np.max(np.abs(Vd)[:, None, :] * A64[None, :, :], axis=2)
    _check("sp_tmul", *both(sp_tmul), Vd @ X64.T, sp_floor)


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("family", ["gaussian", "binomial"])
def test_path_against_the_float64_dense_fit(hip, fmt, family):
    """300 x 40, groups of 1, 1, 4, 10 and 24 columns, alpha = 0.8, 10 lambdas: within the float32 routes' 2e-3 of the float64
    fit of the dense design on the same values; full-Gram engines; the KKT excess of the gradient scores over lambda at most
    4 times the float32 dense fit's plus n * eps32 * the largest score."""
    import torch

    n, p = 300, 40
    rng = np.random.default_rng(3)
    X = rng.normal(size=(n, p)).astype(np.float32)
    X = (X.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32) if fmt == "bf16" else X.astype(np.float16).astype(np.float32)
    beta = np.zeros(p)
    beta[[0, 2, 3, 20]] = [1.0, -0.8, 0.5, 0.7]
    eta = X @ beta
    y = eta + 0.3 * rng.normal(size=n) if family == "gaussian" else (rng.uniform(size=n) < 1 / (1 + np.exp(-eta))).astype(float)
    make = (lambda dt: ad.glm.gaussian(y, dtype=dt)) if family == "gaussian" else (lambda dt: ad.glm.binomial(y, dtype=dt))
    t = torch.from_numpy(np.ascontiguousarray(X.T)).to("cuda").to(torch.bfloat16 if fmt == "bf16" else torch.float16).t()
    D = ad.matrix.dense(t)
    assert D._kind == "dense16" and D.dtype == np.float32
    kw = dict(groups=np.array([0, 1, 2, 6, 16]), alpha=0.8, lmda_path_size=10, min_ratio=0.05, early_exit=False, progress_bar=False)
    f32 = dict(kw, tol=1e-7, newton_tol=1e-5)  # (the float32 routes' settings, tests/test_gpu_cons_linear.py: 1e-12 is below float32)
    st = ad.grpnet(D, make(np.float32), **f32)
    s32 = ad.grpnet(ad.matrix.dense(np.asfortranarray(X)), make(np.float32), **f32)
    ref = ad.grpnet(ad.matrix.dense(np.asfortranarray(X.astype(np.float64))), make(np.float64), tol=1e-10, **kw)
    assert st.error == "" and s32.error == "" and ref.error == ""
    assert st.counters["engine_panel"] == 0, st.counters
    assert len(st.lmdas) == len(ref.lmdas) == 10
    db = np.abs(st.betas.toarray() - ref.betas.toarray()).max()
    print(f"  {family} {fmt}: max|dbeta| {db:.3e} (float32 dense {np.abs(s32.betas.toarray() - ref.betas.toarray()).max():.3e})")
    assert db < 2e-3 and np.abs(st.intercepts - ref.intercepts).max() < 2e-3

    def excess(s):
        sc = ad.diagnostic.diagnostic(s).gradient_scores
        return float(np.max(sc - np.asarray(s.lmdas)[:, None])), float(np.max(np.abs(sc)))
    e16, smax = excess(st)
    e32, _ = excess(s32)
    print(f"  {family} {fmt}: KKT excess 16-bit {e16:.3e} float32 dense {e32:.3e}")
    assert e16 <= 4 * max(e32, 0.0) + n * EPS32 * smax


def _refusals():
    y = np.zeros(8)
    box = lambda: [ad.constraint.box(np.array([-1.0]), np.array([1.0])) for _ in range(3)]  # noqa: E731
    return {
        "kronecker_eye": (lambda D, t: ad.matrix.kronecker_eye(D, 2), "kronecker_eye"),
        "standardize": (lambda D, t: ad.matrix.standardize(D), "standardize"),
        "concatenate": (lambda D, t: ad.matrix.concatenate([D, D], axis=1), "concatenate"),
        "lazy_cov": (lambda D, t: ad.matrix.lazy_cov(D), "lazy_cov"),
        "bvls": (lambda D, t: ad.bvls(D, y, np.full(3, -1.0), np.full(3, 1.0)), "bvls"),
        "constraint": (lambda D, t: ad.grpnet(D, ad.glm.gaussian(y, dtype=np.float32), constraints=box(), progress_bar=False),
                       "constraints are not implemented on a dense design kept 16-bit"),
        "method_cov": (lambda D, t: ad.matrix.dense(t[:3], method="cov"), 'method="cov"'),
        "int8": (lambda D, t: ad.matrix.dense(t.to(__import__("torch").int8)), "torch.int8.*torch.bfloat16"),
    }


@pytest.mark.parametrize("what", list(_refusals()))
def test_what_a_16_bit_design_refuses(hip, what):
    import torch

    t = torch.arange(24, dtype=torch.float32, device="cuda").reshape(3, 8).t().to(torch.bfloat16)  # (8, 3), F-contiguous
    D = ad.matrix.dense(t)
    fn, match = _refusals()[what]
    with pytest.raises(RuntimeError, match=match):
        fn(D, t)
    out = np.empty(3, np.float32)  # the design is as it was
    D.mul(np.ones(8, np.float32), np.ones(8, np.float32), out)
    assert np.array_equal(out, t.float().sum(dim=0).cpu().numpy())
