"""Creation of a phased-ancestry design (matrix.snp_phased_calldata: the (n, 2s) code table uploaded, the compressed arrays built
on the device by kernels_phased.hip) against the route without it: the numpy expansion of the same calls into a
scipy.sparse.csc_matrix, then matrix.sparse(..., resident="csc") (host tocsr, validation and upload of both compressed forms).
Same data, same process, f64, the generator's default ratios:

    n = 100 000, s = 2 000, A = 8: 16 000 columns, about 7e7 stored entries

    python scripts/bench_phased.py [--n 100000] [--s 2000] [--A 8] [--repeats 3] [--out profiles/phased_build.txt]

Wall-clock time of each whole call (both end synchronised), alternating the two routes, median over `--repeats`; the scipy
route is split into the expansion and the matrix.sparse call.  One full sweep of each design through adelie_hip_bench_sweep
(HIP events) checks that the two designs are the same thing: the arrays are compared as well.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time
import warnings

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import adelie_amd as ad  # noqa: E402
from adelie_amd import _abi  # noqa: E402
from adelie_amd.matrix import _csc_download  # noqa: E402


def expand_csc(cal, anc, A, dtype):
    """The expansion without the dense (n, s A) array: one triplet per mutated haplotype; duplicates add up to the 2s."""
    n = cal.shape[0]
    i, c = np.nonzero(cal == 1)
    col = (c // 2) * A + anc[i, c]
    return sp.csc_matrix((np.ones(i.size, dtype=dtype), (i, col)), shape=(n, cal.shape[1] // 2 * A))


def sweep_ms(b, X, window):
    ms = C.c_double()
    b.check(b.fn("bench_sweep")(X._handle, 3, C.byref(ms)))
    b.check(b.fn("bench_sweep")(X._handle, 10, C.byref(ms)))
    reps = int(min(5000, max(10, window * 1e3 / max(ms.value, 1e-4))))
    out = []
    for _ in range(3):
        b.check(b.fn("bench_sweep")(X._handle, reps, C.byref(ms)))
        out.append(ms.value)
    return float(np.median(out)), reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--s", type=int, default=2_000)
    ap.add_argument("--A", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of sweep launches per timing")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, s, A, dtype = args.n, args.s, args.A, np.float64
    b = _abi.hip_backend()
    t0 = time.perf_counter()
    d = ad.data.snp_phased_ancestry(n, s, A, seed=0)
    cal, anc = d["X"], d["ancestries"]
    t_gen = time.perf_counter() - t0
    ad.matrix.snp_phased_calldata(cal[:1000], anc[:1000], A)            # warm-up: library load, code objects, first allocations
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ad.matrix.sparse(expand_csc(cal[:1000], anc[:1000], A, dtype), resident="csc")
    t_dev, t_exp, t_up = [], [], []
    X = Y = None
    for _ in range(args.repeats):
        X = Y = None                                                     # (one design of each route alive at a time)
        t0 = time.perf_counter()
        X = ad.matrix.snp_phased_calldata(cal, anc, A)
        t_dev.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        E = expand_csc(cal, anc, A, dtype)
        t_exp.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            Y = ad.matrix.sparse(E, resident="csc")
        t_up.append(time.perf_counter() - t0)
        del E
    same = all(np.array_equal(a, c) for a, c in zip(_csc_download(X), _csc_download(Y)))
    nnz = int(b.fn("design_nnz")(X._handle))
    sw_x, reps = sweep_ms(b, X, args.window)
    sw_y, _ = sweep_ms(b, Y, args.window)
    med = lambda v: float(np.median(v))  # noqa: E731
    r = dict(n=n, s=s, A=A, cols=s * A, nnz=nnz, dtype="float64", repeats=args.repeats, generate_s=t_gen, table_bytes=2 * n * s,
             device_build_s=med(t_dev), device_build_all=[round(x, 3) for x in t_dev],
             numpy_expand_s=med(t_exp), numpy_expand_all=[round(x, 3) for x in t_exp],
             sparse_upload_s=med(t_up), sparse_upload_all=[round(x, 3) for x in t_up],
             scipy_route_s=med(t_exp) + med(t_up), ratio=(med(t_exp) + med(t_up)) / med(t_dev),
             arrays_equal=bool(same), sweep_ms_device_built=sw_x, sweep_ms_scipy_built=sw_y, sweep_reps=reps)
    print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("Creation of a phased-ancestry design on one MI355X (scripts/bench_phased.py): matrix.snp_phased_calldata (code table\n"
                    "uploaded, compressed arrays built on the device) against the numpy expansion to scipy.sparse.csc_matrix followed by\n"
                    f"matrix.sparse(resident=\"csc\").  Same data, one process, wall clock of the whole calls, median of {args.repeats} "
                    "alternating repeats.\n\n"
                    f"n = {n}, s = {s}, A = {A}: {s * A} columns, {nnz} stored entries, f64; code table {2 * n * s / 1e6:.0f} MB "
                    f"(generator: {t_gen:.1f} s)\n"
                    f"  snp_phased_calldata (host pack, upload, device build, finishing half)  {r['device_build_s']:.3f} s   {r['device_build_all']}\n"
                    f"  numpy expansion to csc_matrix                                         {r['numpy_expand_s']:.3f} s   {r['numpy_expand_all']}\n"
                    f"  matrix.sparse(resident=\"csc\") on it (tocsr, checks, upload, finishing)  {r['sparse_upload_s']:.3f} s   {r['sparse_upload_all']}\n"
                    f"  scipy route / device route = {r['ratio']:.1f}x\n"
                    f"  the six arrays of the two designs are equal: {same}\n"
                    f"  one full sweep (adelie_hip_bench_sweep, HIP events, median of 3 rounds of {reps} launches): "
                    f"{sw_x:.4f} ms on the device-built design, {sw_y:.4f} ms on the scipy-built one\n")


if __name__ == "__main__":
    main()
