"""solver.pinball on one MI355X with a large sparse constraint set, float64: the same matrix solved once through
matrix.sparse(method="constraint") (kept sparse in HBM) and once through matrix.dense(method="constraint").

    python scripts/bench_pinball_sparse.py [--m 2000000] [--d 512] [--per-row 8] [--pen 0.1] [--reps 1] [--out profiles/pinball_sparse.txt]

A has --per-row stored entries ~ N(0, 1) in every row, at seeded random columns: one column drawn uniformly from each of
--per-row equal strata of the d columns (so the columns of a row are distinct and every row holds exactly that many entries).
S = X'X and v = X'y of a (2 d + 8, d) Gaussian X and the penalties pen * U(0, 1) are those of scripts/bench_pinball.py.  The
dense copy is scattered on the device from the same entries, so no (m, d) host array is formed.  For both routes: resident bytes
of A, seconds per call of ad.pinball (wall clock: set-up, solve, download of the state), the three device phases of the solve
(HIP events on its stream: sweeps, AS / H builds, the fit kernel), stored entries per second of the full sweep, and whether the
two trajectories agree.  One JSON line per route; --out writes the table that profiles/pinball_sparse.txt holds.  No pass mark."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import adelie_amd as ad  # noqa: E402
import pinball_checks as pc  # noqa: E402


def make_rows(m, d, per_row, seed):
    """The CSR arrays of A: per_row entries per row, one column from each of per_row equal strata of [0, d)."""
    rs = np.random.RandomState(seed)
    edges = np.linspace(0, d, per_row + 1).astype(np.int64)
    cols = np.empty((m, per_row), dtype=np.int32)
    for k in range(per_row):
        cols[:, k] = rs.randint(edges[k], edges[k + 1], size=m)
    vals = rs.normal(size=(m, per_row))
    indptr = np.arange(0, (m + 1) * per_row, per_row, dtype=np.int64)
    return sp.csr_matrix((vals.ravel(), cols.ravel(), indptr), shape=(m, d))


def solve(A, S, v, pneg, ppos, reps):
    ad.pinball(A, S, v, pneg, ppos, max_iters=2)  # warm-up: code objects, the device buffers
    best, state = np.inf, None
    for _ in range(reps):
        t0 = time.perf_counter()
        s = ad.pinball(A, S, v, pneg, ppos)
        t = time.perf_counter() - t0
        if t < best:
            best, state = t, s
    return best, state


def figures(route, resident, nnz, best, state):
    bm = state.benchmark
    sweep_ms = bm["t_sweep_ms"]
    return dict(route=route, resident_bytes=int(resident), seconds=best, solve_seconds=state.total_time, iters=state.iters,
                n_kkt=state.n_kkt, ns=int(state.screen_set_size), active=int(state.active_set_size), error=state.error,
                t_sweep_ms=sweep_ms, t_gram_ms=bm["t_gram_ms"], t_fit_ms=bm["t_fit_ms"], changed_visits=int(bm["n_changed"]),
                stored_entries_per_s=state.n_kkt * nnz / max(sweep_ms, 1e-9) * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=2000000)
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--per-row", type=int, default=8)
    ap.add_argument("--pen", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    m, d, k = args.m, args.d, args.per_row
    if not 1 <= k <= d:
        ap.error("--per-row must be in [1, d]")
    mat = make_rows(m, d, k, 0)
    nnz = int(mat.nnz)
    _, S, v, _, _ = pc.gen(1, d, 0, args.pen)
    rs = np.random.RandomState(1)
    pneg, ppos = args.pen * rs.uniform(0, 1, m), args.pen * rs.uniform(0, 1, m)

    A_sp = ad.matrix.sparse(mat, method="constraint")
    # (the two compressed forms: 12 bytes per stored entry each way, and the two pointer arrays)
    resident_sp = 2 * nnz * 12 + (m + 1) * 8 + (d + 1) * 8
    best_sp, st_sp = solve(A_sp, S, v, pneg, ppos, args.reps)
    sparse = figures("sparse", resident_sp, nnz, best_sp, st_sp)
    print(json.dumps(sparse), flush=True)
    del A_sp

    At = torch.zeros(m, d, dtype=torch.float64, device="cuda")  # (m, d) row-major: adopted in place
    rows = torch.from_numpy(np.repeat(np.arange(m, dtype=np.int64), np.diff(mat.indptr))).to("cuda")
    At[rows, torch.from_numpy(mat.indices.astype(np.int64)).to("cuda")] = torch.from_numpy(mat.data).to("cuda")
    del rows
    torch.cuda.synchronize()
    A_de = ad.matrix.dense(At, method="constraint")
    best_de, st_de = solve(A_de, S, v, pneg, ppos, args.reps)
    dense = figures("dense", m * d * 8, nnz, best_de, st_de)
    dense["sweep_gb_per_s"] = st_de.n_kkt * m * d * 8 / max(dense["t_sweep_ms"], 1e-9) / 1e6
    print(json.dumps(dense), flush=True)

    def members(s):
        return list(s.screen_set[:s.screen_set_size]), list(s.active_set[:s.active_set_size])

    agree = dict(same_sets=bool(members(st_sp) == members(st_de)), same_iters=bool(st_sp.iters == st_de.iters),
                 same_n_kkt=bool(st_sp.n_kkt == st_de.n_kkt), max_abs_dbeta=float(np.max(np.abs(st_sp.beta - st_de.beta))),
                 max_abs_beta=float(np.max(np.abs(st_de.beta))), max_abs_dresid=float(np.max(np.abs(st_sp.resid - st_de.resid))),
                 max_abs_resid=float(np.max(np.abs(st_de.resid))))
    print(json.dumps(agree), flush=True)
    if args.out:
        def block(f):
            return (f"{f['route']} route: A resident in {f['resident_bytes'] / 1e9:.3f} GB; {f['seconds']:.3f} s per call of ad.pinball "
                    f"(set-up + solve + download), {f['solve_seconds']:.3f} s inside adelie_hip_pinball_solve\n"
                    f"  iters {f['iters']}, n_kkt {f['n_kkt']}, ns {f['ns']}, active {f['active']}, changed visits {f['changed_visits']}"
                    f"{', error: ' + f['error'] if f['error'] else ''}\n"
                    f"  device time (HIP events): t_sweep_ms {f['t_sweep_ms']:.3f}, t_gram_ms {f['t_gram_ms']:.3f}, t_fit_ms {f['t_fit_ms']:.3f}\n"
                    f"  full sweeps: {f['n_kkt']} of {nnz} stored entries, {f['stored_entries_per_s'] / 1e9:.2f} G stored entries / s"
                    + (f" ({f['sweep_gb_per_s']:.0f} GB/s of m * d * 8 bytes per sweep)" if "sweep_gb_per_s" in f else
                       f" ({12 * f['stored_entries_per_s'] / 1e9:.0f} GB/s of 12 bytes per stored entry)") + "\n")

        with open(args.out, "w") as f:
            f.write(f"solver.pinball on one MI355X, float64, A ({m}, {d}) with {k} stored entries ~ N(0, 1) per row at seeded random "
                    f"columns (one per stratum of {d}/{k} columns), {nnz} in all; S = X'X of a ({2 * d + 8}, {d}) Gaussian X, penalties "
                    f"{args.pen} * U(0, 1), defaults (kappa = min(m, d), tol 1e-7).\nscripts/bench_pinball_sparse.py, best of {args.reps} "
                    f"solve(s) per route after one warm-up call; the same matrix through matrix.sparse(method=\"constraint\") and, scattered "
                    f"on the device, through matrix.dense(method=\"constraint\").\n\n" + block(sparse) + "\n" + block(dense) + "\n"
                    f"trajectories: same ordered screen and active sets {agree['same_sets']}, same iters {agree['same_iters']}, same n_kkt "
                    f"{agree['same_n_kkt']}; max |beta_sparse - beta_dense| {agree['max_abs_dbeta']:.3e} (max |beta| {agree['max_abs_beta']:.3e}), "
                    f"max |resid_sparse - resid_dense| {agree['max_abs_dresid']:.3e} (max |resid| {agree['max_abs_resid']:.3e})\n"
                    f"t_gram_ms sparse / dense {sparse['t_gram_ms'] / max(dense['t_gram_ms'], 1e-9):.3f}; t_sweep_ms sparse / dense "
                    f"{sparse['t_sweep_ms'] / max(dense['t_sweep_ms'], 1e-9):.3f}\n")


if __name__ == "__main__":
    main()
