"""diagnostic.DiagnosticCov on one MI355X, float64: the L = 100 gradients v - A beta_l of a solved gaussian_cov path through one
lambda-batched product (A.mul_batch, adelie_hip_design_cov_mul_batch) against L single A.mul calls.

    python scripts/bench_cov_diag.py [--handle sparse|dense|both] [--single] [--no-diag] [--reps 10] [--out FILE]
                                     [--p-sparse 1000000] [--per-col 500] [--p-dense 20000] [--n-dense 4000]

Handles: "sparse" is the banded matrix of scripts/bench_cov_sparse.py shape B kept sparse in HBM (p = 10^6, 501 stored entries
per column); "dense" is lazy_cov of a Gaussian (n, p) X / sqrt(n), p = 20 000, dense in HBM.  v = A beta + 0.01 N(0, 1) with 100
coefficients of size 1 to 2; a 100-lambda lasso path (min_ratio 0.05, tol 1e-7, early_exit off) gives the coefficient rows.

Legs, each repeated --reps times after one warm-up, timed with HIP events recorded on the handle's stream around the calls
(the uploads, the kernels and the downloads of a leg; the host work between two calls of the loop is inside, as it is for a
caller) and by the wall clock; median, minimum and maximum are printed:
    single   L calls of A.mul, one per row, into the rows of one reused (L, p) array (entries the parent commit has; --single
             runs this leg only); the subtraction from v, which the caller of single products does on the host, is not timed
    batched  one A.mul_batch(B, v, out=) into a reused, touched (L, p) array: the leg the condition below compares with single
    batched_new_array  the same into a new array per call, as DiagnosticCov calls it: a copy down into pageable memory that was
             never touched pays for the first touch of every page inside the copy (both routes of DiagnosticCov pay it)
    download a device-to-host copy of an (L, p) float64 array into touched pageable memory, the size batched brings back
and DiagnosticCov(state) end to end by the wall clock, with the batched product and with the per-lambda fallback (new arrays
on both routes).
Byte models beside the times: kept sparse ceil(L / 8) (12 nnz + 8 p 8 2) batched against L (12 nnz + 16 p) single; dense
sum over batches |U_b| p 8 against sum over rows nnz(beta_l) p 8.  One JSON line per handle; --out appends it to a file.
The condition printed: batched median <= single median + (single max - single min)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import adelie_amd as ad  # noqa: E402
from bench_cov_sparse import make_banded, true_beta  # noqa: E402

KW = dict(lmda_path_size=100, min_ratio=0.05, tol=1e-7, early_exit=False, progress_bar=False)
LB = 8


def stream_of(A):
    import torch

    ptr = A._backend.fn("design_stream")(A._handle)
    return torch.cuda.ExternalStream(int(ptr)) if ptr else torch.cuda.default_stream()


def timed(fn, stream, reps):
    """(event ms, wall ms) per repetition of fn(), after one warm-up call"""
    import torch

    fn()
    ev, wall = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(e0.elapsed_time(e1))
    return ev, wall


def stats(xs):
    return dict(median=float(np.median(xs)), min=float(np.min(xs)), max=float(np.max(xs)))


def measure(name, A, v, nnz, args):
    import torch

    p = A.cols()
    ad.gaussian_cov(A, v, **dict(KW, lmda_path_size=3))  # warm-up: code objects, the device buffers
    st = ad.gaussian_cov(A, v, **KW)
    B = st.betas.tocsr()
    L = B.shape[0]
    rows = [(B[l].indices.astype(np.int64), B[l].data.astype(np.float64)) for l in range(L)]
    counts = np.diff(B.indptr)
    stream = stream_of(A)
    out = np.empty((L, p))
    res = dict(handle=name, p=p, nnz=int(nnz), L=L, error=st.error, active_last=int(counts[-1]), mean_active=float(counts.mean()),
               reps=args.reps)

    def single():
        for l, (idx, val) in enumerate(rows):
            A.mul(idx, val, out[l])

    ev, wall = timed(single, stream, args.reps)
    res["single_event_ms"], res["single_wall_ms"] = stats(ev), stats(wall)
    ref = v[None] - out  # (outside the timed window: host work that the batched entry does on the device)
    unions = [len(np.unique(B[b:b + LB].indices)) for b in range(0, L, LB)]
    if name == "sparse":
        res["bytes_single"] = float(L) * (12.0 * nnz + 16.0 * p)
        res["bytes_batched"] = float(-(-L // LB)) * (12.0 * nnz + 8.0 * p * LB * 2)
    else:
        res["bytes_single"] = float(counts.sum()) * p * 8
        res["bytes_batched"] = float(sum(unions)) * p * 8
        res["mean_batch_overlap"] = float(counts.sum()) / max(sum(unions), 1)
    if not args.single:
        got = {}

        def batched():
            got["out"] = A.mul_batch(B, v)

        buf = np.zeros((L, p))
        buf[:] = 1.0  # (touched, as single's `out` is after its warm-up: no copy down meets a page for the first time)
        ev, wall = timed(lambda: A.mul_batch(B, v, out=buf), stream, args.reps)
        res["batched_event_ms"], res["batched_wall_ms"] = stats(ev), stats(wall)
        res["same_bits"] = bool(np.array_equal(buf, ref))
        del buf
        ev, _ = timed(batched, stream, args.reps)
        res["batched_new_array_event_ms"] = stats(ev)
        res["same_bits"] = res["same_bits"] and bool(np.array_equal(got["out"], ref))
        spread = res["single_event_ms"]["max"] - res["single_event_ms"]["min"]
        res["condition_batched_not_slower"] = bool(res["batched_event_ms"]["median"] <= res["single_event_ms"]["median"] + spread)
        res["speedup_event"] = res["single_event_ms"]["median"] / res["batched_event_ms"]["median"]
        dev = torch.zeros((L, p), dtype=torch.float64, device="cuda")
        host = torch.empty((L, p), dtype=torch.float64)
        ev, _ = timed(lambda: host.copy_(dev), torch.cuda.current_stream(), args.reps)
        res["download_event_ms"] = stats(ev)
        res["download_share_of_batched"] = res["download_event_ms"]["median"] / res["batched_event_ms"]["median"]
        del dev, host
        if args.no_diag:
            return res
        backend = type(A._backend)
        has = backend.has

        def diag_ms():
            ts = []
            ad.diagnostic.DiagnosticCov(st)
            for _ in range(max(3, args.reps // 2)):
                t0 = time.perf_counter()
                d = ad.diagnostic.DiagnosticCov(st)
                ts.append((time.perf_counter() - t0) * 1e3)
            return stats(ts), d

        res["diagnostic_batched_wall_ms"], d1 = diag_ms()
        backend.has = lambda self, n: n != "design_cov_mul_batch" and has(self, n)
        try:
            res["diagnostic_fallback_wall_ms"], d2 = diag_ms()
        finally:
            backend.has = has
        res["diagnostic_same_bits"] = bool(np.array_equal(d1.gradients, d2.gradients))
        lm = np.asarray(st.lmdas)[:, None]
        inactive = B.toarray() == 0 if p <= 50000 else None
        if inactive is not None:
            res["max_inactive_score_over_lmda"] = float((d1.gradient_scores / lm)[inactive].max())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--handle", choices=["sparse", "dense", "both"], default="both")
    ap.add_argument("--single", action="store_true", help="only the leg of single A.mul calls (entries the parent commit has)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--p-sparse", type=int, default=1000000)
    ap.add_argument("--per-col", type=int, default=500)
    ap.add_argument("--p-dense", type=int, default=20000)
    ap.add_argument("--n-dense", type=int, default=4000)
    ap.add_argument("--no-diag", action="store_true", help="skip the DiagnosticCov end-to-end legs")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    if args.handle in ("sparse", "both"):
        p = args.p_sparse
        S = make_banded(p, args.per_col)
        beta, noise = true_beta(p, 1)
        v = S @ beta + noise
        A = ad.matrix.sparse(S, method="cov", resident="csc")
        del S
        lines.append(json.dumps(measure("sparse", A, v, A.nnz, args)))
        print(lines[-1], flush=True)
        del A
    if args.handle in ("dense", "both"):
        p, n = args.p_dense, args.n_dense
        X = np.asfortranarray(np.random.RandomState(0).normal(size=(n, p)) / np.sqrt(n))
        A = ad.matrix.lazy_cov(X)
        beta, noise = true_beta(p, 1)
        nz = np.flatnonzero(beta)
        v = np.empty(p)
        A.mul(nz, beta[nz], v)
        v += noise
        lines.append(json.dumps(measure("dense", A, v, p * p, args)))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
