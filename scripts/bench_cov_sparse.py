"""solver.gaussian_cov on one MI355X with the covariance matrix kept sparse in HBM, float64.

    python scripts/bench_cov_sparse.py --shape A [--p 100000] [--block 500] [--reps 5] [--out FILE]
    python scripts/bench_cov_sparse.py --shape B [--p 1000000] [--per-col 500] [--reps 3] [--out FILE]

Shape A: block-diagonal, blocks of --block (B'B / m of a Gaussian (m, block) B, m = block + 100), the same matrix through
matrix.block_diag(method="cov", resident="csc") and through matrix.block_diag(method="cov") (dense in HBM, pasted into a (p, p)
host array first).  Shape B: banded, --per-col stored entries per column (one more for an even count: the pattern is symmetric), symmetric and diagonally dominant, kept sparse only
(the dense form of the default size is 8 TB).  v = A beta + 0.01 N(0, 1) with 100 coefficients of size 1 to 2; a 100-lambda
lasso path, min_ratio 0.05, tol 1e-7, early_exit off.

Per route: resident bytes, seconds per path (wall clock of ad.gaussian_cov, every repetition listed), the mean time of the
per-lambda grad launch (HIP events: t_sweep_ms / n_sweep_launches; on the sparse route the zeroing and filling of w are
inside) with its bytes per second, (12 nnz + 24 p) / t, and the total time of the gathers into the screen Gram matrix
(t_gram_ms).  Shape A also prints the run-to-run spread of the dense route and whether the sparse route's best path time
stays within the dense route's best plus that spread.  One JSON line per route; --out appends the lines to a file.  No pass mark
beyond that one condition."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import adelie_amd as ad  # noqa: E402

KW = dict(lmda_path_size=100, min_ratio=0.05, tol=1e-7, early_exit=False, progress_bar=False)


def true_beta(p, seed):
    rs = np.random.RandomState(seed)
    beta = np.zeros(p)
    beta[rs.choice(p, 100, replace=False)] = rs.choice([-1.0, 1.0], 100) * rs.uniform(1, 2, 100)
    return beta, 0.01 * rs.normal(size=p)


def make_blocks(p, q, seed):
    rs = np.random.RandomState(seed)
    out = []
    for o in range(0, p, q):
        w = min(q, p - o)
        B = rs.normal(size=(w + 100, w))
        out.append(np.asfortranarray(B.T @ B / (w + 100)))
    return out


def make_banded(p, per_col, chunk=50000):
    """CSC arrays of the banded matrix: column j stores the rows within per_col // 2 of j inside [0, p) (a symmetric pattern:
    per_col + 1 entries for an even per_col); the diagonal is 1 and A[i, j] = 0.9 cos(0.37 (i + j) + 0.11 |i - j|) / per_col
    off it, so every row is diagonally dominant."""
    lo = np.maximum(np.arange(p, dtype=np.int64) - per_col // 2, 0)
    hi = np.minimum(np.arange(p, dtype=np.int64) + per_col // 2 + 1, p)
    counts = hi - lo
    indptr = np.concatenate([[0], np.cumsum(counts)])
    nnz = int(indptr[-1])
    indices = np.empty(nnz, dtype=np.int32)
    data = np.empty(nnz)
    for c0 in range(0, p, chunk):
        c1 = min(p, c0 + chunk)
        e0, e1 = int(indptr[c0]), int(indptr[c1])
        cols = np.repeat(np.arange(c0, c1, dtype=np.int64), counts[c0:c1])
        rows = np.arange(e0, e1, dtype=np.int64) - np.repeat(indptr[c0:c1] - lo[c0:c1], counts[c0:c1])
        vals = 0.9 * np.cos(0.37 * (rows + cols) + 0.11 * np.abs(rows - cols)) / per_col
        vals[rows == cols] = 1.0
        indices[e0:e1] = rows
        data[e0:e1] = vals
    A = sp.csc_matrix((data, indices, indptr), shape=(p, p))
    A.has_sorted_indices = True
    return A


def run(A, v, reps):
    ad.gaussian_cov(A, v, **dict(KW, lmda_path_size=3))  # warm-up: code objects, the device buffers
    times, state = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        s = ad.gaussian_cov(A, v, **KW)
        times.append(time.perf_counter() - t0)
        state = s
    return times, state


def figures(shape, route, p, nnz, resident, times, st):
    tm = st.timers
    n_grad = max(tm["n_sweep_launches"], 1)
    grad_ms = tm["t_sweep_ms"] / n_grad
    out = dict(shape=shape, route=route, p=p, nnz=nnz, resident_bytes=int(resident), path_seconds=[round(t, 4) for t in times],
               best_path_seconds=min(times), lmdas=len(st.lmdas), error=st.error, screen=len(st.screen_set),
               active=int(st.active_set_size), grad_launches=int(n_grad), mean_grad_ms=grad_ms,
               grad_tb_per_s=(12 * nnz + 24 * p) / max(grad_ms, 1e-9) / 1e9, gather_ms_total=tm["t_gram_ms"],
               gather_launches=int(tm["n_gram_launches"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["A", "B"], required=True)
    ap.add_argument("--p", type=int, default=None)
    ap.add_argument("--block", type=int, default=500)
    ap.add_argument("--per-col", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(json.dumps(d))

    if args.shape == "A":
        p = args.p or 100000
        blocks = make_blocks(p, args.block, 0)
        beta, noise = true_beta(p, 1)
        v = noise.copy()
        o = 0
        for b in blocks:
            v[o:o + len(b)] += b @ beta[o:o + len(b)]
            o += len(b)
        nnz = sum(b.size for b in blocks)
        As = ad.matrix.block_diag(blocks, method="cov", resident="csc")
        assert As.nnz == nnz
        ts, ss = run(As, v, args.reps)
        sparse = figures("A", "sparse", p, nnz, 12 * nnz + 8 * (p + 1), ts, ss)
        emit(sparse)
        del As
        t0 = time.perf_counter()
        Ad = ad.matrix.block_diag(blocks, method="cov")
        build_dense = time.perf_counter() - t0
        td, sd = run(Ad, v, args.reps)
        ld = (p + 31) // 32 * 32
        dense = figures("A", "dense", p, nnz, ld * p * 8, td, sd)
        dense["build_seconds"] = build_dense
        dense["grad_tb_per_s"] = None  # (the dense launch reads the active columns only: not a streaming figure)
        emit(dense)
        spread = max(td) - min(td)
        emit(dict(shape="A", dense_spread_seconds=spread, dense_best=min(td), sparse_best=min(ts),
                  condition_sparse_not_slower=bool(min(ts) <= min(td) + spread),
                  max_abs_dbeta=float(np.abs(ss.betas - sd.betas).max()), same_lmdas=bool(np.array_equal(ss.lmdas, sd.lmdas))))
    else:
        p = args.p or 1000000
        A = make_banded(p, args.per_col)
        beta, noise = true_beta(p, 1)
        v = A @ beta + noise
        As = ad.matrix.sparse(A, method="cov", resident="csc")
        nnz = As.nnz
        ts, ss = run(As, v, args.reps)
        emit(figures("B", "sparse", p, nnz, 12 * nnz + 8 * (p + 1), ts, ss))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
