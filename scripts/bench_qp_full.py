"""adelie_amd.optimization on one MI355X: the NNQP descent (the kind with the most changed visits on these problems) per dtype.

    python scripts/bench_qp_full.py [--reps 7] [--batch 4096] [--big-d 2000] [--out profiles/qp_full.txt]

Problems are those of tests/qp_full_checks.py (X ~ N(0, 1) of (2 d, d) over sqrt(2 d), quad = X'X, v = X'y, x = 0, grad = v;
tol 1e-24 in float64 and 1e-10 in float32).  Three figures per dtype, each the median of --reps timed calls after one warm-up
call, every call from x = 0:
  * one d = 64 solve (wave form): seconds inside the native call (uploads, one launch, downloads) and around .solve()
  * --batch d = 32 problems in one solve_many: seconds per problem
  * one d = --big-d solve (block form) on a quad that is already a device tensor, with the per-coordinate state in LDS and -- via
    the config key qp_full_lds_max_d -- in global memory: seconds per changed visit; the visits are counted by the numpy
    restatement, whose bits the device reproduces (a changed visit reads one slice of quad, d values, and ends with one barrier)
One JSON line per figure; --out writes the table that profiles/qp_full.txt holds.  No pass mark: nothing exists yet to compare
these times with."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import adelie_amd as ad  # noqa: E402
from adelie_amd import _abi  # noqa: E402
import qp_full_checks as qc  # noqa: E402

opt = ad.optimization


def set_config(name, value):
    b = _abi.hip_backend()
    b.check(b.fn("set_config")(name.encode(), float(value)))


def timed(make, run, reps):
    """Medians of (native seconds, wall seconds) of run(make()) over `reps` calls after one warm-up; the last states."""
    native, wall, states = [], [], None
    for k in range(reps + 1):
        states = make()
        t0 = time.perf_counter()
        run(states)
        t = time.perf_counter() - t0
        if k:
            wall.append(t)
            native.append(sum(s.time_elapsed for s in states))
    return statistics.median(native), statistics.median(wall), states


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--big-d", type=int, default=2000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    lines = []
    for dtype in ("float64", "float32"):
        tol = qc.tol_for(dtype)

        def state(P, quad=None):
            return opt.StateNNQPFull(P.quad if quad is None else quad, qc.MAX_ITERS, tol, np.zeros(P.d, dtype=P.dtype), P.v.copy())

        P = qc.problem(128, 64, 0, dtype)
        native, wall, st = timed(lambda: [state(P)], lambda s: s[0].solve(), args.reps)
        one = dict(figure="one d=64 solve", dtype=dtype, native_seconds=native, wall_seconds=wall, iters=st[0].iters)
        print(json.dumps(one), flush=True)

        probs = [qc.problem(64, 32, seed, dtype) for seed in range(args.batch)]
        native, wall, st = timed(lambda: [state(Q) for Q in probs], opt.solve_many, args.reps)
        many = dict(figure=f"{args.batch} d=32 problems in one solve_many", dtype=dtype, native_seconds=native, wall_seconds=wall,
                    seconds_per_problem=native / args.batch, max_iters_seen=max(s.iters for s in st))
        print(json.dumps(many), flush=True)

        d = args.big_d
        B = qc.problem(2 * d, d, 0, dtype)
        stats = {}
        x, grad = np.zeros(d, dtype=B.dtype), B.v.copy()
        iters, _ = qc.solve("nnqp", B.quad, (), B.y_var, qc.MAX_ITERS, tol, x, grad, stats)
        quad_dev = torch.from_numpy(np.ascontiguousarray(B.quad)).to("cuda")
        big = {}
        for form, key in (("lds", 0), ("global", 65)):
            try:
                set_config("qp_full_lds_max_d", key)
                native, wall, st = timed(lambda: [state(B, quad_dev)], lambda s: s[0].solve(), args.reps)
            finally:
                set_config("qp_full_lds_max_d", 0)
            same = bool(st[0].iters == iters and np.array_equal(qc.bits(st[0].x), qc.bits(x)))
            big[form] = dict(figure=f"one d={d} solve, state in {form}", dtype=dtype, native_seconds=native, wall_seconds=wall,
                             iters=st[0].iters, changed_visits=stats["changed"], us_per_changed_visit=native * 1e6 / stats["changed"],
                             slice_bytes=d * B.dtype.itemsize, same_bits_as_restatement=same)
            print(json.dumps(big[form]), flush=True)
        lines.append(
            f"{dtype}\n"
            f"  one d = 64 solve (wave form, {one['iters']} sweeps): {one['native_seconds'] * 1e6:.1f} us inside the native call, "
            f"{one['wall_seconds'] * 1e6:.1f} us around .solve()\n"
            f"  {args.batch} d = 32 problems in one solve_many (at most {many['max_iters_seen']} sweeps): "
            f"{many['native_seconds'] * 1e3:.3f} ms inside the native call = {many['seconds_per_problem'] * 1e6:.3f} us per problem; "
            f"{many['wall_seconds'] * 1e3:.3f} ms around solve_many\n"
            + "".join(
                f"  one d = {d} solve (block form, state in {form}; {v['iters']} sweeps, {v['changed_visits']} changed visits of "
                f"{v['slice_bytes']} bytes each): {v['native_seconds'] * 1e3:.3f} ms = {v['us_per_changed_visit']:.3f} us per changed "
                f"visit; bits equal to the restatement's: {v['same_bits_as_restatement']}\n" for form, v in big.items()))
    if args.out:
        with open(args.out, "w") as f:
            f.write("adelie_amd.optimization.StateNNQPFull on one MI355X; problems of tests/qp_full_checks.py (quad = X'X, X ~ N(0, 1) of "
                    f"(2 d, d) over sqrt(2 d)), tol 1e-24 (float64) / 1e-10 (float32).\nscripts/bench_qp_full.py, medians of {args.reps} "
                    "calls after one warm-up call.  The d = " + str(args.big_d) + " quad is a device tensor (only the vectors cross "
                    "PCIe); the others are uploaded in the call.\n\n" + "\n".join(lines))


if __name__ == "__main__":
    main()
