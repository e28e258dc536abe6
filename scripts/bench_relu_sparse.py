"""Full sweep of a convex-relu design over a sparse base, kept sparse (matrix.convex_relu(..., resident="csc")): the structured
kernel (kernels_relu_sparse.hip, ADELIE_HIP_RELU_SWEEP=1: off Z's compressed columns, the packed mask and v) against the
compressed-column sweep of the same expanded design (=0, the baseline: the sweep of every design kept sparse), through
adelie_hip_bench_sweep (HIP events around `reps` launches on resident buffers, no host copies), alternating the two routes in
one process.  Two shapes generated here, f64:

  gated    n = 200 000, d = 5 000, Z density 1 %,  m = 32
  signed   n = 100 000, d = 500,   Z density 10 %, m = 8

    python scripts/bench_relu_sparse.py [--scale 1.0] [--window 0.25] [--rounds 5] [--out profiles/relu_sparse_sweep.txt]

Each route's launches per round are chosen so that a round lasts about `--window` seconds.  Also times the build on the
device against matrix._relu_expand_sparse on the host plus matrix.sparse(..., resident="csc") on its result.  Prints one JSON
line per shape; --out also writes the table that profiles/relu_sparse_sweep.txt holds.  The structured sweep is the default of
the library only if it is faster than the baseline on both shapes by more than the round-to-round spread
(common.hpp: kReluSparseSweepDefault)."""
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
from adelie_amd.matrix import _relu_expand_sparse, _relu_sparse_sweep_shape  # noqa: E402

HOOK = "ADELIE_HIP_RELU_SWEEP"


def time_route(b, X, hook, reps):
    os.environ[HOOK] = hook
    ms = C.c_double()
    b.check(b.fn("bench_sweep")(X._handle, reps, C.byref(ms)))
    return ms.value


def run_shape(name, n, d, density, m, gated, args, b, seed):
    rng = np.random.default_rng(seed)
    # (a Generator, not a legacy RandomState: that one permutes all n * d cells to draw the stored ones)
    Z = sp.random(n, d, density=density, format="csc", dtype=np.float64, random_state=rng, data_rvs=lambda k: rng.normal(size=k))
    mask = np.asfortranarray((Z @ rng.normal(size=(d, m))) >= 0)   # D_k = 1[Z u_k >= 0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t0 = time.perf_counter()
        X = ad.matrix.convex_relu(Z, mask, gated=gated, resident="csc")
        build_dev = time.perf_counter() - t0
        t0 = time.perf_counter()
        S = _relu_expand_sparse(Z, mask, gated)
        build_host_expand = time.perf_counter() - t0
        t0 = time.perf_counter()
        Xs = ad.matrix.sparse(S, resident="csc")
        build_host_upload = time.perf_counter() - t0
    nnz = int(b.fn("design_nnz")(X._handle))
    assert nnz == S.nnz == int(b.fn("design_nnz")(Xs._handle))
    del Xs, S
    P = X.shape[1]
    reps, t = {}, {"0": [], "1": []}
    for hook in ("0", "1"):                                # warm-up of both code objects, then the launches per round
        time_route(b, X, hook, 3)
        reps[hook] = int(min(20000, max(10, args.window * 1e3 / max(time_route(b, X, hook, 10), 1e-4))))
    for _ in range(args.rounds):
        for hook in ("0", "1"):
            t[hook].append(time_route(b, X, hook, reps[hook]))
    # the same sums on both routes (reordered floating-point additions only)
    v, w = rng.normal(size=n), np.ones(n)
    outs = {}
    for hook in ("0", "1"):
        os.environ[HOOK] = hook
        outs[hook] = np.empty(P)
        X.mul(v, w, outs[hook])
    os.environ.pop(HOOK)
    tile_rows, tiles, words = _relu_sparse_sweep_shape(n, m)
    base_ms, relu_ms = float(np.median(t["0"])), float(np.median(t["1"]))
    spread = max(max(t[h]) - min(t[h]) for h in ("0", "1"))
    return dict(shape=name, n=n, d=d, m=m, density=density, gated=gated, P=P, nnz_Z=int(Z.nnz), nnz_X=nnz, rounds=args.rounds,
                reps_base=reps["0"], reps_relu=reps["1"], tile_rows=tile_rows, tiles=tiles, words=words,
                base_ms=base_ms, base_ms_all=[round(x, 4) for x in t["0"]], relu_ms=relu_ms,
                relu_ms_all=[round(x, 4) for x in t["1"]], spread_ms=spread, speedup=base_ms / relu_ms,
                faster_beyond_spread=bool(base_ms - relu_ms > spread),
                build_device_s=build_dev, build_host_expand_s=build_host_expand, build_host_upload_s=build_host_upload,
                max_abs_diff=float(np.abs(outs["0"] - outs["1"]).max()), max_abs_out=float(np.abs(outs["0"]).max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="scales n of both shapes (a quick look: 0.1)")
    ap.add_argument("--window", type=float, default=0.25, help="seconds of launches per route and round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    b = _abi.hip_backend()
    rows = []
    for k, (name, n, d, density, m, gated) in enumerate((("gated", 200_000, 5_000, 0.01, 32, True),
                                                          ("signed", 100_000, 500, 0.10, 8, False))):
        rows.append(run_shape(name, max(1, int(n * args.scale)), d, density, m, gated, args, b, k))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("Full sweep of a convex-relu design over a sparse base, kept sparse (matrix.convex_relu(..., resident=\"csc\")) on one\n"
                    "MI355X: structured kernel (ADELIE_HIP_RELU_SWEEP=1, kernels_relu_sparse.hip) against the compressed-column sweep of the\n"
                    "same expanded design (=0).  scripts/bench_relu_sparse.py, adelie_hip_bench_sweep, HIP events, median of "
                    f"{args.rounds} alternating\nrounds of about {args.window} s of launches per route, one process.\n\n")
            for r in rows:
                f.write(f"{r['shape']}: n = {r['n']}, d = {r['d']}, Z density {r['density']:.0%}, m = {r['m']}, P = {r['P']}, float64; "
                        f"nnz(Z) = {r['nnz_Z']}, nnz(X) = {r['nnz_X']}; grid {r['d']} columns of Z x {r['tiles']} row tiles of "
                        f"{r['tile_rows']} rows x {r['words']} mask words\n"
                        f"  compressed-column sweep  {r['base_ms']:.4f} ms per launch   rounds of {r['reps_base']} launches {r['base_ms_all']}\n"
                        f"  structured sweep         {r['relu_ms']:.4f} ms per launch   rounds of {r['reps_relu']} launches {r['relu_ms_all']}\n"
                        f"  baseline / structured = {r['speedup']:.2f}x   round-to-round spread {r['spread_ms']:.4f} ms   "
                        f"max|difference of the two results| = {r['max_abs_diff']:.3e} (largest |result| {r['max_abs_out']:.3e})\n"
                        f"  build: on the device {r['build_device_s']:.2f} s (Z uploaded, counted, filled, csc_finish); on the host "
                        f"{r['build_host_expand_s']:.2f} s (_relu_expand_sparse) + {r['build_host_upload_s']:.2f} s (matrix.sparse of the result)\n\n")
            ok = all(r["faster_beyond_spread"] for r in rows)
            f.write("Rule for kReluSparseSweepDefault (common.hpp): true only if the structured route is faster on both shapes by more than "
                    f"the round-to-round spread -> {'true' if ok else 'false'}.\n")


if __name__ == "__main__":
    main()
