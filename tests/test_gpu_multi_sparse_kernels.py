"""The K-wide kernels over a base kept sparse (``kernels_multi_sparse.hip``), one launcher at a time through
``adelie_hip_multi_sparse_piece_test``, against numpy in ``longdouble`` on the dense expansion ``[1, X]`` of the test matrix.

Bound, valid for any order of summation (atomics included): ``|got - ref| <= (m + 2) u sum|terms|`` with ``m`` the number of
non-zero terms of that output and ``u`` the unit roundoff.  Entries are small integers and vectors multiples of 1/8, so the
reference's own rounding is nil against the bound."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

LD = np.longdouble
P = 37
EMPTY, FULL = 5, 6  # special base columns; with n = 700 the full column has more than 256 entries
DTYPES = [np.float64, np.float32]
KS = [1, 3, 8, 9]   # below, at and past a response chunk of 8


def _matrix(n, dtype):
    rng = np.random.RandomState(n)
    D = rng.randint(-3, 4, size=(n, P)) * (rng.uniform(size=(n, P)) < 0.2)
    D[:, EMPTY] = 0
    D[:, FULL] = rng.randint(1, 4, size=n)
    return D.astype(dtype)


def _vec(rng, shape, dtype, lo=-32, hi=33):
    return (rng.randint(lo, hi, size=shape) / 8.0).astype(dtype)


def _call(hip, mode, D, K, icpt, rb=0, th=0, **a):
    from adelie_amd import _abi
    dtype = D.dtype.type
    Mc, Mr = sp.csc_matrix(D), sp.csr_matrix(D)
    Mc.sort_indices(), Mr.sort_indices()
    keep = dict(cptr=Mc.indptr.astype(np.int64), cidx=Mc.indices.astype(np.int32), cval=Mc.data.astype(dtype),
                rptr=Mr.indptr.astype(np.int64), rcol=Mr.indices.astype(np.int32), rval=Mr.data.astype(dtype))
    s = _abi.MultiSparsePiece()
    s.dtype, s.mode = _abi.dtype_code(dtype), mode
    s.n, s.p, s.K, s.icpt, s.nnz, s.rb, s.th = D.shape[0], D.shape[1], K, icpt, Mc.nnz, rb, th
    for k, v in {**keep, **a}.items():
        if isinstance(v, np.ndarray):
            assert v.flags.c_contiguous and v.dtype in (dtype, np.int32, np.int64), k
            setattr(s, k, v.ctypes.data)
        else:
            setattr(s, k, v)
    hip.check(hip.fn("multi_sparse_piece_test")(C.byref(s)))


def _expansion(D, icpt):
    E = D.astype(LD)
    return np.concatenate([np.ones((D.shape[0], 1), LD), E], axis=1) if icpt else E


def _check(got, ref, absterms, m, dtype):
    u = np.finfo(dtype).eps / 2
    bound = (np.asarray(m, LD) + 2) * u * np.asarray(absterms, LD)
    err = np.abs(got.astype(LD) - ref)
    assert np.all(err <= bound), (float(err.max()), np.argwhere(err > bound)[:5].tolist())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("icpt", [0, 1])
@pytest.mark.parametrize("n,rb,th", [(193, 0, 0), (193, 64, 0), (193, 64, 64), (700, 64, 64)])
def test_sweep(hip, dtype, K, icpt, n, rb, th):
    from adelie_amd import _abi
    D = _matrix(n, dtype)
    rng = np.random.RandomState(K)
    v = _vec(rng, n * K, dtype)
    out = np.full((P + icpt) * K, 77, dtype)
    _call(hip, _abi.MULTI_SPARSE_SWEEP, D, K, icpt, rb, th, v=v, out=out)
    E, V = _expansion(D, icpt), v.astype(LD).reshape(K, n)
    _check(out.reshape(P + icpt, K), E.T @ V.T, np.abs(E).T @ np.abs(V).T, (E != 0).T.astype(LD) @ (V != 0).T.astype(LD), dtype)


def _lists(case, rng, K, icpt):
    """dcol, nz and cols of a step: view columns c = u K + l, the K responses of a feature next to each other."""
    nfeat, ncol = P + icpt, (P + icpt) * K
    full, empty = FULL + icpt, EMPTY + icpt
    feats = [0, full, empty, 9, 12, 20]  # (0: the ones feature with icpt, a plain column without)
    every = lambda fs, keep=lambda u, l: True: np.array([u * K + l for u in fs for l in range(K) if keep(u, l)], np.int32)
    some = every(feats)
    if case == "nz0":
        return some[:7], 0, some
    if case == "nz_short":
        return some, min(4, len(some)), some
    if case == "partial":  # a feature present for only some of its responses, in both lists
        part = every(feats, lambda u, l: (u + l) % 2 == 0)
        return part, len(part), every(feats, lambda u, l: (u + l) % 3 != 1)
    if case == "shared":   # the full column, the ones and two more columns touch the same rows
        sh = every([0, full, 9, 12])
        return sh, len(sh), some
    if case == "cols1":
        return some[:3], 3, every([full])[:1]
    order = rng.permutation(nfeat)                 # "colsmax": the launcher's maximum of both lists
    allc = every(order)
    return allc[:128], min(128, ncol), allc[:256]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("icpt", [0, 1])
@pytest.mark.parametrize("case,n", [("nz0", 193), ("nz_short", 193), ("partial", 193), ("shared", 700), ("cols1", 193), ("colsmax", 193)])
def test_step(hip, dtype, K, icpt, case, n):
    from adelie_amd import _abi
    D = _matrix(n, dtype)
    rng = np.random.RandomState(K + 10)
    dcol, nz, cols = _lists(case, rng, K, icpt)
    dlt = _vec(rng, len(dcol), dtype, -8, 9)
    w, r0 = _vec(rng, n * K, dtype, 1, 9), _vec(rng, n * K, dtype)
    r, g = r0.copy(), np.full(len(cols), 77, dtype)
    _call(hip, _abi.MULTI_SPARSE_STEP, D, K, icpt, w=w, r=r, dcol=dcol, dlt=dlt, n_dcol=len(dcol), nz=nz, cols=cols, nb_cols=len(cols), gblk=g)
    E = _expansion(D, icpt)
    R, A, M = r0.astype(LD).reshape(K, n).copy(), np.abs(r0.astype(LD)).reshape(K, n), np.ones((K, n), LD)
    for m in range(min(nz, 128)):
        u, l = divmod(int(dcol[m]), K)
        t = LD(dlt[m]) * E[:, u]
        R[l] -= t
        A[l] += np.abs(t)
        M[l] += t != 0
    _check(r.reshape(K, n), R, A, M, dtype)
    # the gradient is checked against the device's own residual: its bound is that of one dot product
    WR = w.astype(LD).reshape(K, n) * r.astype(LD).reshape(K, n)
    ref = np.array([E[:, c // K] @ WR[c % K] for c in cols])
    absr = np.array([np.abs(E[:, c // K]) @ np.abs(WR[c % K]) for c in cols])
    cnt = np.array([np.count_nonzero(E[:, c // K] * WR[c % K]) + 1 for c in cols])  # (+ 1: the product w r rounds once)
    _check(g, ref, absr, cnt, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("icpt", [0, 1])
@pytest.mark.parametrize("n", [193, 700])
@pytest.mark.parametrize("weights", ["uniform", "per_response"])
def test_gram(hip, dtype, icpt, n, weights):
    from adelie_amd import _abi
    D = _matrix(n, dtype)
    rng = np.random.RandomState(n + icpt)
    K = 3
    W = np.full((K, n), 0.25, dtype) if weights == "uniform" else _vec(rng, (K, n), dtype, 1, 9)
    ucols = np.array([0, FULL + icpt, EMPTY + icpt] + list(rng.permutation(np.arange(8, P))[:20] + icpt), np.int32)  # (0: ones with icpt)
    M, ldc = len(ucols), 128
    E = _expansion(D, icpt)[:, ucols]
    for l in range(1 if weights == "uniform" else K):
        Cm = np.full(M * ldc, 77, dtype)
        _call(hip, _abi.MULTI_SPARSE_GRAM, D, K, icpt, w=np.ascontiguousarray(W[l]), ucols=ucols, M=M, ldc=ldc, C=Cm)
        wl = W[l].astype(LD)
        got = Cm.reshape(M, ldc)[:, :M].T  # C[a + b ldc]
        _check(got, E.T @ (wl[:, None] * E), np.abs(E).T @ (wl[:, None] * np.abs(E)), (E != 0).T.astype(LD) @ (E != 0).astype(LD) + 1, dtype)  # (+ 1: w x rounds once)
        assert np.all(Cm.reshape(M, ldc)[:, M:] == 77)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("icpt", [0, 1])
@pytest.mark.parametrize("sign,n", [(1.0, 193), (-1.0, 700)])
def test_axpy(hip, dtype, K, icpt, sign, n):
    from adelie_amd import _abi
    D = _matrix(n, dtype)
    rng = np.random.RandomState(K + 20)
    dcol, _, _ = _lists("partial", rng, K, icpt)
    nz = len(dcol) - 1  # the count is read on the device: the last entry is not applied
    dlt, r0 = _vec(rng, len(dcol), dtype, -8, 9), _vec(rng, n * K, dtype)
    r = r0.copy()
    _call(hip, _abi.MULTI_SPARSE_AXPY, D, K, icpt, r=r, dcol=dcol, dlt=dlt, n_dcol=len(dcol), nz=nz, sign=sign)
    E = _expansion(D, icpt)
    R, A, M = r0.astype(LD).reshape(K, n).copy(), np.abs(r0.astype(LD)).reshape(K, n), np.ones((K, n), LD)
    for m in range(nz):
        u, l = divmod(int(dcol[m]), K)
        t = LD(sign) * LD(dlt[m]) * E[:, u]
        R[l] += t
        A[l] += np.abs(t)
        M[l] += t != 0
    _check(r.reshape(K, n), R, A, M, dtype)
