"""Multi-response fits on a design kept sparse: the kept-sparse route (kernels_multi_sparse.hip) against the expanded route
(set_configs("multi_keep_sparse", False): the view over the dense copy, made once here and timed apart), alternated in one
process.  profiles/multi_sparse.txt.

    python scripts/bench_multi_sparse.py [--reps 5] [--reach]

One JSON line per measurement.  Times are wall clock of ad.grpnet per path after one warm-up call of each route (median and
min-max over --reps), sweeps are HIP-event times per launch (adelie_hip_bench_sweep, 20 launches)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import adelie_amd as ad  # noqa: E402


def rand_csc(rng, n, p, nnz_per_col):
    rows = rng.randint(0, n, size=(p, nnz_per_col))
    rows.sort(axis=1)
    M = sp.csc_matrix((rng.normal(size=p * nnz_per_col), rows.ravel(), np.arange(p + 1, dtype=np.int64) * nnz_per_col), shape=(n, p))
    M.sum_duplicates()
    return M


def responses(rng, M, K, k=30):
    B = np.zeros((M.shape[1], K))
    B[rng.choice(M.shape[1], k, replace=False)] = rng.normal(size=(k, K))
    eta = M @ B
    Y = eta + 0.5 * rng.normal(size=eta.shape)
    return Y, np.eye(K)[np.argmax(eta + rng.gumbel(size=eta.shape), axis=1)]


def kept(M):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return ad.matrix.sparse(M, resident="csc")


def sweep_ms(X, reps=20):
    b, ms = X._backend, C.c_double()
    b.check(b.fn("bench_sweep")(X._handle, reps, C.byref(ms)))
    return ms.value


def owned():
    """Device bytes owned by all live design handles."""
    from adelie_amd import _abi
    return int(_abi.hip_backend().fn("design_owned_bytes")())


def timed(f, reps):
    f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        st = f()
        ts.append(time.perf_counter() - t0)
    return st, dict(median_s=statistics.median(ts), min_s=min(ts), max_s=max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reach", action="store_true")
    a = ap.parse_args()
    rng = np.random.RandomState(0)
    K = 4
    kw = dict(lmda_path_size=50, min_ratio=0.1, early_exit=False, progress_bar=False)
    if a.reach:
        n, p = 1_000_000, 100_000
        M = rand_csc(rng, n, p, 1000)
        _, cls = responses(rng, M, K)
        X = kept(M)
        st, t = timed(lambda: ad.grpnet(X, ad.glm.multinomial(cls), **kw), max(1, a.reps // 2))
        print(json.dumps(dict(run="reach", n=n, p=p, nnz=int(M.nnz), K=K, family="multinomial", resident_bytes=owned(), error=st.error,
                              lmdas=len(st.lmdas), active=int((st.betas[-1] != 0).sum()), **t)), flush=True)
        return
    n, p = 200_000, 20_000
    M = rand_csc(rng, n, p, n // 200)
    Y, cls = responses(rng, M, K)
    X = kept(M)
    kept_bytes = owned()
    ad.set_configs("multi_keep_sparse", False)
    t0 = time.perf_counter()
    Xd = ad.matrix.kronecker_eye(X, K)._base  # the expanded copy: what the switch builds for every view; made once here
    ad.set_configs("multi_keep_sparse")
    print(json.dumps(dict(run="resident", n=n, p=p, nnz=int(M.nnz), kept_sparse_bytes=kept_bytes, expanded_bytes=owned() - kept_bytes,
                          expand_seconds=time.perf_counter() - t0)), flush=True)
    for family, glm in (("multigaussian", lambda: ad.glm.multigaussian(Y)), ("multinomial", lambda: ad.glm.multinomial(cls))):
        res = {}
        for route in ("kept_sparse", "expanded", "kept_sparse", "expanded"):  # alternated
            st, t = timed(lambda: ad.grpnet(X if route == "kept_sparse" else Xd, glm(), **kw), a.reps)
            res.setdefault(route, []).append((st, t))
        sa, sb = res["kept_sparse"][-1][0], res["expanded"][-1][0]
        for route, runs in res.items():
            for st, t in runs:
                print(json.dumps(dict(run="path", family=family, route=route, K=K, lmdas=len(st.lmdas), error=st.error,
                                      active=int((st.betas[-1] != 0).sum()), **t)), flush=True)
        print(json.dumps(dict(run="path_diff", family=family, max_abs_dbeta=float(abs(sa.betas - sb.betas).max()))), flush=True)
    # one K-wide full sweep against K single-response sparse sweeps and against the dense multi sweep
    Vs, Vd = ad.matrix.kronecker_eye(X, K), ad.matrix.kronecker_eye(Xd, K)
    for _ in range(2):
        print(json.dumps(dict(run="sweep", K=K, kwide_sparse_ms=sweep_ms(Vs), single_sparse_ms=sweep_ms(X), K_single_sparse_ms=K * sweep_ms(X),
                              kwide_dense_ms=sweep_ms(Vd))), flush=True)


if __name__ == "__main__":
    main()
