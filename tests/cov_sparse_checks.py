"""Shared generators of the tests of the covariance matrix kept sparse (matrix.sparse(method="cov", resident="csc")):
banded positive semi-definite matrices with exact zeros outside the band, a block-diagonal one, one with a column that stores
only its diagonal entry, and the path arguments every test runs under.  Everything is cached and read-only."""
import functools

import numpy as np
import scipy.sparse as sp

import adelie_amd as ad

# (n, p, w, G): p = 1 | a few entries per column | ~47 per column | screen values beyond 256 (the multi-CU Gram engines) |
# groups of 10 for the group engines | columns of 399 entries (more than one pass of a 64-lane group) | fully dense
GRID = [(40, 1, 1, 1), (60, 23, 5, 23), (400, 301, 24, 301), (900, 700, 90, 700), (800, 640, 80, 64), (900, 700, 200, 700),
        (300, 150, 150, 30)]
GRID32 = GRID[:4]
GROUPED = (800, 640, 80, 64)
WIDE = (900, 700, 200, 700)         # largest column count > 256
DENSE = (300, 150, 150, 30)
BLOCKS = (3, 17, 40, 70)
PATH = dict(lmda_path_size=30, min_ratio=0.05, early_exit=False, progress_bar=False)


def path_kwargs(case, dtype=np.float64):
    """Arguments of the 30-lambda path of a grid case (tol = 1e-12 in f64; 1e-7 in f32, below which the convergence measure is
    rounding noise -- what tests/test_cov.py runs f32 paths under)."""
    n, p, w, G = case
    kw = dict(PATH, groups=np.arange(0, p, p // G), tol=1e-12 if dtype == np.float64 else 1e-7)
    if G != p:
        kw.update(alpha=0.7)
        if dtype != np.float64:
            kw.update(newton_tol=1e-5)
    return kw


def _frozen(*xs):
    for x in xs:
        x.setflags(write=False)
    return xs


@functools.lru_cache(maxsize=None)
def banded(n, p, w, seed=0):
    """X (n, p): row i holds w normal values in a window that slides from column 0 to p - w.  Returns (A, v) with A = X'X / n
    (positive semi-definite, exact zeros outside a band of 2w - 1) and v = X'y / n, y from a third of the coefficients."""
    rng = np.random.RandomState(seed)
    X = np.zeros((n, p))
    for i in range(n):
        c0 = int(round(i * (p - w) / max(n - 1, 1)))
        X[i, c0:c0 + w] = rng.normal(size=w)
    beta = rng.normal(size=p) * (np.arange(p) % 3 == 0)
    y = X @ beta + rng.normal(size=n)
    return _frozen(X.T @ X / n, X.T @ y / n)


@functools.lru_cache(maxsize=None)
def problem(case, dtype=np.float64):
    """(A, v) of a grid case rounded to dtype, A F-ordered."""
    n, p, w, G = case
    A, v = banded(n, p, w, seed=n + p)
    return _frozen(np.asfortranarray(A.astype(dtype)), v.astype(dtype))


@functools.lru_cache(maxsize=None)
def block_diag_blocks(dtype=np.float64):
    rng = np.random.RandomState(8)
    out = []
    for q in BLOCKS:
        B = rng.normal(size=(q + 5, q))
        out.append(np.asfortranarray((B.T @ B / (q + 5)).astype(dtype)))
    return _frozen(*out)


@functools.lru_cache(maxsize=None)
def block_diag_matrix(dtype=np.float64):
    """The blocks of 3, 17, 40 and 70 pasted on the diagonal, and a v."""
    blocks = block_diag_blocks(dtype)
    p = sum(BLOCKS)
    A = np.zeros((p, p), dtype=dtype, order="F")
    o = 0
    for b in blocks:
        A[o:o + len(b), o:o + len(b)] = b
        o += len(b)
    return _frozen(A, np.random.RandomState(9).normal(size=p).astype(dtype))


LONE = 150  # the column of lone_diag_matrix that stores only its diagonal entry


@functools.lru_cache(maxsize=None)
def lone_diag_matrix():
    """The p = 301 matrix with row and column LONE struck out but for the diagonal."""
    A = problem(GRID[2])[0].copy()
    A[LONE, :] = 0
    A[:, LONE] = 0
    A[LONE, LONE] = 1.0
    return _frozen(np.asfortranarray(A))[0]


def col_counts(A):
    """Stored entries per column of csc_matrix(A)."""
    return np.diff(sp.csc_matrix(A).indptr)


def dot_bound(absA, absw, counts, dtype):
    """(k + 1) eps sum |a||b| for the dots of the columns of A with w, k the terms of a dot (the bound form of
    tests/test_gpu_pinball_sparse.py); absA (p, m), absw (p,), counts (m,)."""
    return (counts + 1) * np.finfo(dtype).eps * (absw @ absA)


@functools.lru_cache(maxsize=None)
def oracle_path(case, dtype=np.float64):
    """The CPU oracle's covariance path of a grid case."""
    from oracle import oracle as orc

    orc.build()
    A, v = problem(case, dtype)
    return ad.gaussian_cov(orc.cov_dense(A), v, **path_kwargs(case, dtype))


def screen_values(state, case):
    n, p, w, G = case
    return len(state.screen_set) * (p // G)
