"""Full sweep of a one-hot / interaction design: the structured kernel (kernels_factor.hip, ADELIE_HIP_FACTOR_SWEEP=1) against the
dense sweep on the identical expanded matrix (=0), through adelie_hip_bench_sweep (HIP events around `reps` launches on
resident buffers, no host copies), alternating the two routes in one process.  Two shapes:

  interaction   n rows, ten continuous + ten discrete features with 2..11 levels, every pair with feature 0 and with feature 10
  one_hot       n rows, fifty discrete features with 2..11 levels

    python scripts/bench_factor.py [--n 1000000] [--dtype float64] [--reps 200] [--rounds 5] [--out profiles/factor_sweep.txt]

Prints one JSON line per shape; --out also writes the table that profiles/factor_sweep.txt holds.  The structured sweep is the
default of the library only if it is at least as fast as the dense sweep on both shapes (common.hpp: kFactorSweepDefault)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import adelie_amd as ad  # noqa: E402
from adelie_amd import _abi  # noqa: E402

CHUNK = 16  # kFactorChunk: columns of one block a workgroup of the structured sweep owns


def make_table(n, levels, dtype, rng):
    Z = np.empty((n, len(levels)), dtype=dtype, order="F")
    for j, L in enumerate(levels):
        Z[:, j] = rng.normal(size=n) if L <= 0 else rng.integers(0, L, size=n)
    return Z


def time_route(b, X, hook, reps):
    os.environ["ADELIE_HIP_FACTOR_SWEEP"] = hook
    ms = C.c_double()
    b.check(b.fn("bench_sweep")(X._handle, reps, C.byref(ms)))
    return ms.value


def run_shape(name, X, one_hot, args, b):
    n, P = X.shape
    s = np.dtype(X.dtype).itemsize
    b.check(b.fn("bench_sweep")(X._handle, 3, C.byref(C.c_double())))  # warm-up of both code objects
    time_route(b, X, "1", 3)
    t = {"0": [], "1": []}
    for _ in range(args.rounds):
        for hook in ("0", "1"):
            t[hook].append(time_route(b, X, hook, args.reps))
    # the same sums on both routes (reordered floating-point additions only)
    rng = np.random.default_rng(1)
    v, w = rng.normal(size=n).astype(X.dtype), np.ones(n, dtype=X.dtype)
    outs = {}
    for hook in ("0", "1"):
        os.environ["ADELIE_HIP_FACTOR_SWEEP"] = hook
        outs[hook] = np.empty(P, dtype=X.dtype)
        X.mul(v, w, outs[hook])
    os.environ.pop("ADELIE_HIP_FACTOR_SWEEP")
    chunks = int(np.sum((np.asarray(X.group_sizes) + CHUNK - 1) // CHUNK))
    dense_bytes = n * P * s + n * s                       # the expanded matrix once, v once
    fact_bytes = chunks * n * s * (2 if one_hot else 3)   # per chunk: one or two columns of Z, and v (mostly from L2)
    d_ms, f_ms = float(np.median(t["0"])), float(np.median(t["1"]))
    return dict(shape=name, n=n, d=int(len(X._levels)), P=P, blocks=int(len(X.groups)), chunks=chunks, dtype=np.dtype(X.dtype).name,
                reps=args.reps, rounds=args.rounds, dense_ms=d_ms, dense_ms_all=[round(x, 4) for x in t["0"]],
                factor_ms=f_ms, factor_ms_all=[round(x, 4) for x in t["1"]], speedup=d_ms / f_ms,
                dense_bytes=dense_bytes, factor_bytes=fact_bytes, dense_GBps=dense_bytes / d_ms / 1e6,
                factor_requested_GBps=fact_bytes / f_ms / 1e6, factor_entries_per_ns=n * P / f_ms / 1e6,
                max_abs_diff=float(np.abs(outs["0"] - outs["1"]).max()), max_abs_out=float(np.abs(outs["0"]).max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dtype", default="float64")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dtype = np.dtype(args.dtype).type
    b = _abi.hip_backend()
    rng = np.random.default_rng(0)
    rows = []
    # interaction-heavy: 10 continuous + 10 discrete (2..11 levels), every pair with feature 0 and with feature 10
    levels = np.concatenate([np.zeros(10, dtype=int), np.arange(2, 12)])
    Z = make_table(args.n, levels, dtype, rng)
    X = ad.matrix.interaction(Z, {0: None, 10: None}, levels)
    rows.append(run_shape("interaction", X, False, args, b))
    print(json.dumps(rows[-1]), flush=True)
    del X, Z
    # pure one-hot: fifty discrete features
    levels = 2 + (np.arange(50) % 10)
    Z = make_table(args.n, levels, dtype, rng)
    X = ad.matrix.one_hot(Z, levels)
    rows.append(run_shape("one_hot", X, True, args, b))
    print(json.dumps(rows[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("Full sweep of a factor design on one MI355X: structured kernel (ADELIE_HIP_FACTOR_SWEEP=1) against the dense sweep on\n"
                    "the identical expanded matrix (=0).  scripts/bench_factor.py, adelie_hip_bench_sweep, HIP events, median of "
                    f"{args.rounds} alternating rounds of {args.reps} launches.\n\n")
            for r in rows:
                f.write(f"{r['shape']}: n = {r['n']}, d = {r['d']}, P = {r['P']} ({r['blocks']} blocks, {r['chunks']} chunks), {r['dtype']}\n"
                        f"  dense sweep       {r['dense_ms']:.4f} ms per launch   must read {r['dense_bytes'] / 1e6:.1f} MB "
                        f"(n*P + n values)  -> {r['dense_GBps']:.0f} GB/s   rounds {r['dense_ms_all']}\n"
                        f"  structured sweep  {r['factor_ms']:.4f} ms per launch   requests  {r['factor_bytes'] / 1e6:.1f} MB "
                        f"(per chunk: its columns of Z and v) -> {r['factor_requested_GBps']:.0f} GB/s requested, "
                        f"{r['factor_entries_per_ns']:.1f} entries/ns   rounds {r['factor_ms_all']}\n"
                        f"  dense / structured = {r['speedup']:.2f}x   max|difference of the two results| = {r['max_abs_diff']:.3e} "
                        f"(largest |result| {r['max_abs_out']:.3e})\n\n")


if __name__ == "__main__":
    main()
