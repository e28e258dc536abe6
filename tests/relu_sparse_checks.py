"""Inputs and references shared by the tests of matrix.convex_relu over a sparse base (test_relu_sparse_host.py,
test_gpu_relu_sparse.py).  Needs no device."""
import numpy as np
from scipy.sparse import csc_matrix, csr_matrix


def make_inputs(n, d, m, dtype, density=0.3, dead_row=False, seed=0):
    """A sparse Z (csc) and a mask with the special rows and columns: column 1 of Z is empty (d >= 2) and row n // 2 of Z is
    empty (n >= 2); mask column 0 is all false and the last one all true (m >= 2); with ``dead_row`` row n - 1 has every gate
    false (then the last mask column is true everywhere else)."""
    rng = np.random.RandomState(seed + n + 7 * d + 13 * m)
    Z = rng.normal(size=(n, d)) * (rng.uniform(size=(n, d)) < density)
    if d >= 2:
        Z[:, 1] = 0
    if n >= 2:
        Z[n // 2, :] = 0
    mask = rng.uniform(size=(n, m)) < 0.5
    if m >= 2:
        mask[:, 0], mask[:, m - 1] = False, True
    else:
        mask[:, 0] = np.arange(n) % 3 != 1
    if dead_row:
        mask[n - 1, :] = False
    return csc_matrix(Z.astype(dtype)), np.asfortranarray(mask)


def stored_entries(Z, mask, gated):
    """(gated ? 1 : 2) * sum_i popcount(mask[i, :]) * nnz(Z[i, :])"""
    R = csr_matrix(Z)
    R.eliminate_zeros()
    return (1 if gated else 2) * int((mask.sum(axis=1).astype(np.int64) * np.diff(R.indptr).astype(np.int64)).sum())


def canonical(S, dtype):
    """The canonical CSC and CSR of a scipy matrix: sorted, duplicates summed, no explicit zeros."""
    C = csc_matrix(S, dtype=dtype)
    C.sum_duplicates()
    C.eliminate_zeros()
    C.sort_indices()
    R = C.tocsr()
    R.sort_indices()
    return C, R
