"""Full sweep of a convex-relu design (matrix.convex_relu): the structured kernel (kernels_relu.hip, ADELIE_HIP_RELU_SWEEP=1: the
(d, m) matrix product Z^T (mask o v) on the matrix cores) against the dense sweep on the identical expanded matrix (=0), through
adelie_hip_bench_sweep (HIP events around `reps` launches on resident buffers, no host copies), alternating the two routes in
one process.  Two shapes, f64:

  gated    n = 100 000, d = 64,  m = 64:  P = 4 096
  signed   n = 100 000, d = 100, m = 50:  P = 10 000 (the headline benchmark's 100k x 10k)

    python scripts/bench_relu.py [--n 100000] [--dtype float64] [--window 0.25] [--rounds 5] [--out profiles/relu_sweep.txt]

Each route's launches per round are chosen so that a round lasts about `--window` seconds.  Prints one JSON line per shape;
--out also writes the table that profiles/relu_sweep.txt holds.  The structured sweep is the default of the library only if it
is at least as fast as the dense sweep on both shapes (common.hpp: kReluSweepDefault)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import adelie_amd as ad  # noqa: E402
from adelie_amd import _abi  # noqa: E402
from adelie_amd.matrix import _RELU_MT, _RELU_TILE, _relu_sweep_shape  # noqa: E402

HOOK = "ADELIE_HIP_RELU_SWEEP"


def time_route(b, X, hook, reps):
    os.environ[HOOK] = hook
    ms = C.c_double()
    b.check(b.fn("bench_sweep")(X._handle, reps, C.byref(ms)))
    return ms.value


def run_shape(name, n, d, m, gated, args, b, rng):
    dtype = np.dtype(args.dtype).type
    Z = np.asfortranarray(rng.normal(size=(n, d)).astype(dtype))
    mask = np.asfortranarray(Z @ rng.normal(size=(d, m)).astype(dtype) >= 0)   # D_k = 1[Z u_k >= 0]
    X = ad.matrix.convex_relu(Z, mask, gated=gated)
    P = X.shape[1]
    s = np.dtype(dtype).itemsize
    reps, t = {}, {"0": [], "1": []}
    for hook in ("0", "1"):                                # warm-up of both code objects, then the launches per round
        time_route(b, X, hook, 3)
        reps[hook] = int(min(20000, max(10, args.window * 1e3 / max(time_route(b, X, hook, 10), 1e-4))))
    for _ in range(args.rounds):
        for hook in ("0", "1"):
            t[hook].append(time_route(b, X, hook, reps[hook]))
    # the same sums on both routes (reordered floating-point additions only)
    v, w = rng.normal(size=n).astype(dtype), np.ones(n, dtype=dtype)
    outs = {}
    for hook in ("0", "1"):
        os.environ[HOOK] = hook
        outs[hook] = np.empty(P, dtype=dtype)
        X.mul(v, w, outs[hook])
    os.environ.pop(HOOK)
    d_tiles, m_groups, nslice, rps = _relu_sweep_shape(n, d, m)
    dense_bytes = n * P * s + n * s                        # the expanded matrix once, v once
    # what the structured route must read: Z once per group of mask tiles, the mask once per tile of Z, v once; and the
    # partial sums written and read back
    relu_bytes = m_groups * n * d * s + d_tiles * n * m + n * s + 2 * nslice * m * d * s
    flops = 2.0 * n * d * m                                # the product Z^T (mask o v) itself
    flops_issued = 2.0 * n * (d_tiles * _RELU_TILE) * (-(-m // _RELU_TILE) * _RELU_TILE)   # with the tiles' zero fill
    d_ms, r_ms = float(np.median(t["0"])), float(np.median(t["1"]))
    return dict(shape=name, n=n, d=d, m=m, gated=gated, P=P, dtype=np.dtype(dtype).name, rounds=args.rounds,
                reps_dense=reps["0"], reps_relu=reps["1"], d_tiles=d_tiles, m_groups=m_groups, nslice=nslice,
                rows_per_slice=rps, mask_tiles_per_wave=_RELU_MT,
                dense_ms=d_ms, dense_ms_all=[round(x, 4) for x in t["0"]], relu_ms=r_ms,
                relu_ms_all=[round(x, 4) for x in t["1"]], speedup=d_ms / r_ms,
                dense_bytes=dense_bytes, dense_GBps=dense_bytes / d_ms / 1e6,
                relu_bytes=relu_bytes, relu_GBps=relu_bytes / r_ms / 1e6,
                relu_flops=flops, relu_TFLOPs=flops / r_ms / 1e9, relu_issued_TFLOPs=flops_issued / r_ms / 1e9,
                max_abs_diff=float(np.abs(outs["0"] - outs["1"]).max()), max_abs_out=float(np.abs(outs["0"]).max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--dtype", default="float64")
    ap.add_argument("--window", type=float, default=0.25, help="seconds of launches per route and round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    b = _abi.hip_backend()
    rng = np.random.default_rng(0)
    rows = []
    for name, d, m, gated in (("gated", 64, 64, True), ("signed", 100, 50, False)):
        rows.append(run_shape(name, args.n, d, m, gated, args, b, rng))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("Full sweep of a convex-relu design (matrix.convex_relu) on one MI355X: structured kernel (ADELIE_HIP_RELU_SWEEP=1,\n"
                    "kernels_relu.hip) against the dense sweep on the identical expanded matrix (=0).  scripts/bench_relu.py,\n"
                    f"adelie_hip_bench_sweep, HIP events, median of {args.rounds} alternating rounds of about {args.window} s of "
                    "launches per route, one process.\n\n")
            for r in rows:
                f.write(f"{r['shape']}: n = {r['n']}, d = {r['d']}, m = {r['m']}, P = {r['P']}, {r['dtype']}; grid {r['d_tiles']} tiles of Z x "
                        f"{r['m_groups']} groups of {r['mask_tiles_per_wave']} mask tiles x {r['nslice']} row slices of {r['rows_per_slice']} rows\n"
                        f"  dense sweep       {r['dense_ms']:.4f} ms per launch   must read {r['dense_bytes'] / 1e6:.1f} MB "
                        f"(n*P + n values)  -> {r['dense_GBps']:.0f} GB/s effective   rounds of {r['reps_dense']} launches {r['dense_ms_all']}\n"
                        f"  structured sweep  {r['relu_ms']:.4f} ms per launch   must read {r['relu_bytes'] / 1e6:.1f} MB "
                        f"(Z per mask group, mask per Z tile, v, partial sums) -> {r['relu_GBps']:.0f} GB/s; 2 n d m = "
                        f"{r['relu_flops'] / 1e9:.2f} GFLOP -> {r['relu_TFLOPs']:.2f} TFLOP/s achieved ({r['relu_issued_TFLOPs']:.2f} issued "
                        f"with the tiles' zero fill)   rounds of {r['reps_relu']} launches {r['relu_ms_all']}\n"
                        f"  dense / structured = {r['speedup']:.2f}x   max|difference of the two results| = {r['max_abs_diff']:.3e} "
                        f"(largest |result| {r['max_abs_out']:.3e})\n\n")
            ok = all(r["speedup"] >= 1.0 for r in rows)
            f.write(f"Rule for kReluSweepDefault (common.hpp): true only if the structured route is at least as fast on both shapes -> "
                    f"{'true' if ok else 'false'}.\n")


if __name__ == "__main__":
    main()
