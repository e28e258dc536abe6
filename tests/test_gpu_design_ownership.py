"""Who owns a design handle's device arrays, measured exactly with adelie_hip_design_owned_bytes (the bytes the handles of this
process own; free device memory is device-wide and tells nothing on a shared machine).  A handle that allocates owns what the
constructors' formulas say, a handle that borrows (an alias, an in-place slice, an adopted tensor, the base of a view) owns
nothing of what it shares and frees nothing of it, and every constructor gives back all it took -- also one that throws halfway."""
import ctypes
import gc
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import adelie_amd as ad
from test_gpu_filter_sweep import fsweep, make_problem

pytestmark = pytest.mark.gpu

N, P = 37, 5
LD = (N + 31) // 32 * 32


def owned(hip):
    gc.collect()
    return int(hip.fn("design_owned_bytes")())


def data(dtype=np.float64, seed=0):
    return np.asfortranarray(np.random.RandomState(seed).normal(size=(N, P)).astype(dtype))


def calls(seed=1, p=P):
    return np.random.RandomState(seed).choice(np.array([0, 1, 2, -9], dtype=np.int8), size=(N, p), p=[0.5, 0.3, 0.1, 0.1])


def sparse_data(dtype=np.float64, seed=2):
    rng = np.random.RandomState(seed)
    return sp.csc_matrix(np.where(rng.uniform(size=(N, P)) < 0.3, rng.normal(size=(N, P)), 0.0).astype(dtype))


def mask(m=3, seed=3):
    return np.random.RandomState(seed).uniform(size=(N, m)) < 0.5


def phased(seed=4, s=3, A=2):
    rng = np.random.RandomState(seed)
    return ad.matrix.snp_phased_calldata(rng.randint(0, 2, size=(N, 2 * s)).astype(np.int8), rng.randint(0, A, size=(N, 2 * s)).astype(np.int8), A)


def mul(X):
    rng = np.random.RandomState(9)
    dt = X.dtype
    out = np.empty(X.cols(), dtype=dt)
    X.mul(rng.normal(size=X.rows()).astype(dt), rng.uniform(0.5, 1.5, size=X.rows()).astype(dt), out)
    return out.tobytes()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_dense_owns_its_padded_columns_and_an_adopted_tensor_nothing(hip, dtype):
    import torch

    item = np.dtype(dtype).itemsize
    base = owned(hip)
    X = ad.matrix.dense(data(dtype))
    assert owned(hip) - base == LD * P * item
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        R = ad.matrix.dense(np.ascontiguousarray(data(dtype)))          # row-major: staged and transposed, the stage freed
    assert owned(hip) - base == 2 * LD * P * item
    assert mul(R) == mul(X)
    t = torch.from_numpy(np.ascontiguousarray(data(dtype).T)).cuda().T  # column-major on the device: adopted in place
    T = ad.matrix.dense(t)
    assert owned(hip) - base == 2 * LD * P * item
    mul(T)
    del X, R, T
    assert owned(hip) == base


ALIASED = {
    "dense": lambda: ad.matrix.dense(data()),
    "snp": lambda: ad.matrix.snp_calldata(calls()),
    "sparse_csc": lambda: ad.matrix.sparse(sparse_data(), resident="csc"),
    "one_hot": lambda: ad.matrix.one_hot(np.asfortranarray(calls(p=3).clip(0).astype(np.float64)), levels=[3, 0, 3]),
    "relu_dense": lambda: ad.matrix.convex_relu(data(), mask()),
    "relu_sparse": lambda: ad.matrix.convex_relu(sparse_data(), mask(), resident="csc"),
    "phased": phased,
}


@pytest.mark.parametrize("kind", sorted(ALIASED))
def test_an_alias_owns_nothing_and_frees_nothing(hip, kind):
    X = ALIASED[kind]()
    before = owned(hip)
    want = mul(X)
    a = X.alias()
    assert owned(hip) == before
    assert mul(a) == want
    del a
    assert owned(hip) == before
    assert mul(X) == want


def test_views_own_only_what_they_add(hip):
    for dtype in (np.float64, np.float32):
        item = np.dtype(dtype).itemsize
        for X in (ad.matrix.dense(data(dtype)), ad.matrix.snp_calldata(calls(), dtype=dtype)):
            before = owned(hip)
            want = mul(X)
            V = ad.matrix.standardize(X, centers=np.linspace(-1, 1, P), scales=np.linspace(1, 2, P), lazy=True)
            assert owned(hip) - before == 2 * P * item           # the centres and the inverse scales
            M = ad.matrix.kronecker_eye(X, 3)
            assert owned(hip) - before == 2 * P * item + LD * item   # + the multi-response view's column of ones
            S = ad.matrix.subset(X, np.arange(1, 4), axis=1)     # a contiguous range: sliced in place
            assert S._slice_of is X and owned(hip) - before == 2 * P * item + LD * item
            del V, M, S
            assert owned(hip) == before and mul(X) == want


def test_the_shadow_copy_is_counted_and_dropped(hip, monkeypatch):
    prob = make_problem(N, P, 1, seed=11)
    X, w, r, rsum, xm, groups, gsizes, pen = prob
    base = owned(hip)
    Xd = ad.matrix.dense(X)
    before = owned(hip)
    assert before - base == LD * P * 8
    monkeypatch.setenv("ADELIE_HIP_FILTER_SWEEP", "1")
    fsweep(Xd, w, r, rsum, xm, [0], groups, gsizes, pen, np.inf)
    info = Xd.shadow_info()
    assert Xd.shadow_stats()["state"] == 1 and info["bytes"] > 0
    assert owned(hip) - before == info["bytes"]
    a = Xd.alias()                                               # reads its owner's copy
    fsweep(a, w, r, rsum, xm, [0], groups, gsizes, pen, np.inf)
    assert owned(hip) - before == info["bytes"] and Xd.shadow_stats()["builds"] == 1
    del a
    Xd.drop_shadow()
    assert owned(hip) == before
    fsweep(Xd, w, r, rsum, xm, [0], groups, gsizes, pen, np.inf)  # made again, and freed with the design
    assert owned(hip) - before == info["bytes"]
    del Xd
    assert owned(hip) == base


def test_every_constructor_gives_back_what_it_took(hip, tmp_path):
    M = ad.matrix
    base = owned(hip)
    sym = data()[:P].T @ data()[:P]
    io = ad.io.snp_unphased(str(tmp_path / "a.snpdat"))
    io.write(np.asfortranarray(calls()))
    io.read()
    bed = str(tmp_path / "g.bed")
    ad.io.write_bed(bed, calls())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        made = [
            M.dense(data()), M.dense(sym, method="cov"), M.dense(data(), method="constraint"),
            M.lazy_cov(data()),
            M.sparse(sparse_data(), resident="dense"), M.sparse(sparse_data(), resident="csc"),
            M.sparse(sp.csc_matrix(sym), method="cov", resident="dense"), M.sparse(sp.csc_matrix(sym), method="cov", resident="csc"),
            M.sparse(sp.csr_matrix(sparse_data()), method="constraint"),
            M.snp_calldata(calls()), M.snp_unphased(io), M.snp_bed(bed, N),
            phased(),
            M.one_hot(np.asfortranarray(calls(p=3).clip(0).astype(np.float64)), levels=[3, 0, 3]),
            M.interaction(np.asfortranarray(calls(p=3).clip(0).astype(np.float64)), {0: None}, levels=[3, 0, 3]),
            M.convex_relu(data(), mask()), M.convex_relu(data(), mask(), gated=True),
            M.convex_relu(sparse_data(), mask(), resident="csc"),
            M.block_diag([sym, sym], method="cov"), M.block_diag([sym, sym], method="cov", resident="csc"),
        ]
        D, S = M.dense(data()), M.snp_calldata(calls())
        made += [
            M.standardize(D, lazy=False),
            M.subset(D, [0, 2, 3], axis=1), M.subset(D, [5, 1, 30], axis=0), M.subset(S, [0, 2, 3], axis=1), M.subset(S, [5, 1, 30], axis=0),
            M.concatenate([D, M.dense(data(seed=5))], axis=1), M.concatenate([D, S], axis=0),
            M.concatenate([S, M.snp_calldata(calls(seed=6))], axis=1),
        ]
    assert owned(hip) > base
    del made, D, S
    assert owned(hip) == base


def test_a_constructor_that_throws_after_allocating_leaves_nothing(hip, tmp_path):
    io = ad.io.snp_unphased(str(tmp_path / "a.snpdat"))
    io.write(np.asfortranarray(calls()))
    io.read()
    bad = np.array(io._buffer, copy=True)
    hdr = 17 + 24 * P + 8 * (P + 1)
    assert int(np.frombuffer(bad[17 + 24 * P:17 + 24 * P + 8].tobytes(), dtype=np.uint64)[0]) == hdr   # column 0 starts behind the header
    bad[hdr + 7] = 0xFF   # the top byte of its first category offset: the header passes, the column's decoder refuses
    base = owned(hip)
    h = ctypes.c_void_p()
    assert hip.fn("design_create_snp_unphased")(bad.ctypes.data, bad.size, 1, 0, h) != 0
    assert b"category offset" in hip.fn("last_error")()   # (raised after the packed matrix and the panel were allocated)
    assert owned(hip) == base
