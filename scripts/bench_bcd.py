"""adelie_amd.bcd on one MI355X: batches of group updates through solve_many, one solve, and the host loop they replace.

    python scripts/bench_bcd.py [--reps 10] [--batch 100000] [--out profiles/bcd.txt]

Problems: quad ~ U(0.5, 2), linear ~ N(0, 1), l1 = U(0.2, 0.8) ||linear||, l2 = U(0, 0.5), seeded; tol 1e-12 in float64 and 1e-6
in float32.  Per dtype and solver, with HIP events around the native call (which ends in a stream synchronise), the median and
range of --reps calls after two warm-up calls:
  * --batch problems of d = 8 (team tier), d = 64 (team tier, full wavefront) and d = 512 (wave tier) from host arrays (the call
    uploads quad and linear and downloads beta) and from device tensors (nothing but l1, l2 and iters crosses PCIe)
  * one d = 64 solve
and, in float64, the same problems through a Python loop over the CPU oracle's group update (Newton from h = 0; three runs).
One JSON line per figure; --out writes the table that profiles/bcd.txt holds.  No pass mark: nothing exists yet to compare these
times with."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import adelie_amd as ad  # noqa: E402

TOL = {"float64": 1e-12, "float32": 1e-6}


def problems(B, d, dtype):
    rng = np.random.default_rng(d)
    quad = rng.uniform(0.5, 2.0, (B, d))
    linear = rng.normal(size=(B, d))
    l1 = rng.uniform(0.2, 0.8, B) * np.linalg.norm(linear, axis=1)
    l2 = rng.uniform(0.0, 0.5, B)
    return tuple(np.ascontiguousarray(a, dtype=dtype) for a in (quad, linear, l1, l2))


def timed(call, reps):
    """(median, min, max) milliseconds between two HIP events around call(), and its last result."""
    import torch

    ms, out = [], None
    for k in range(reps + 2):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = call()
        stop.record()
        stop.synchronize()
        if k >= 2:
            ms.append(start.elapsed_time(stop))
    return statistics.median(ms), min(ms), max(ms), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=100000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from oracle import oracle

    assert torch.cuda.is_available(), "no HIP device visible"
    B, lines = args.batch, []

    def show(rec):
        print(json.dumps(rec), flush=True)
        return rec

    for dtype in TOL:
        lines.append(dtype)
        for d in (8, 64, 512):
            quad, linear, l1, l2 = problems(B, d, dtype)
            q_t, v_t = torch.from_numpy(quad).to("cuda"), torch.from_numpy(linear).to("cuda")
            for solver in ("newton", "newton_abs"):
                kw = dict(l1=l1, l2=l2, tol=TOL[dtype], solver=solver)
                for where, q, v in (("host arrays", quad, linear), ("device tensors", q_t, v_t)):
                    med, lo, hi, out = timed(lambda: ad.bcd.solve_many(quad=q, linear=v, **kw), args.reps)
                    r = show(dict(figure=f"{B} problems of d={d}", dtype=dtype, solver=solver, inputs=where, ms_median=med, ms_min=lo,
                                  ms_max=hi, us_per_problem=med * 1e3 / B, max_iters_seen=int(out["iters"].max())))
                    lines.append(f"  {B} x d = {d:<3} {solver:<10} {where:<14} {med:8.3f} ms [{lo:.3f}, {hi:.3f}] = "
                                 f"{r['us_per_problem']:.4f} us per problem (at most {r['max_iters_seen']} steps)")
            if dtype == "float64":
                secs = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    for k in range(B):
                        oracle.bcd_newton(quad[k], linear[k], l1[k], l2[k], tol=TOL[dtype])
                    secs.append(time.perf_counter() - t0)
                r = show(dict(figure=f"{B} problems of d={d}", dtype=dtype, solver="oracle loop on the host", s_median=statistics.median(secs),
                              s_min=min(secs), s_max=max(secs), us_per_problem=statistics.median(secs) * 1e6 / B))
                lines.append(f"  {B} x d = {d:<3} Python loop over the oracle's update (host): {r['s_median'] * 1e3:.1f} ms "
                             f"[{min(secs) * 1e3:.1f}, {max(secs) * 1e3:.1f}] = {r['us_per_problem']:.3f} us per problem")
        quad, linear, l1, l2 = problems(1, 64, dtype)
        for solver in ("newton", "newton_abs"):
            med, lo, hi, out = timed(lambda: ad.bcd.solve(quad=quad[0], linear=linear[0], l1=l1[0], l2=l2[0], tol=TOL[dtype], solver=solver),
                                     args.reps)
            show(dict(figure="one d=64 solve", dtype=dtype, solver=solver, ms_median=med, ms_min=lo, ms_max=hi, iters=out["iters"]))
            lines.append(f"  one d = 64 solve, {solver:<10} {med * 1e3:8.1f} us [{lo * 1e3:.1f}, {hi * 1e3:.1f}] ({out['iters']} steps)")
        if dtype == "float64":
            t0 = time.perf_counter()
            for _ in range(1000):
                oracle.bcd_newton(quad[0], linear[0], l1[0], l2[0], tol=TOL[dtype])
            one = (time.perf_counter() - t0) / 1000
            show(dict(figure="one d=64 solve", dtype=dtype, solver="oracle on the host", us=one * 1e6))
            lines.append(f"  one d = 64 solve, the oracle's update on the host: {one * 1e6:.1f} us (mean of 1000)")
    if args.out:
        with open(args.out, "w") as f:
            f.write("adelie_amd.bcd.solve_many / solve on one MI355X; quad ~ U(0.5, 2), linear ~ N(0, 1), l1 = U(0.2, 0.8) ||linear||, "
                    "l2 = U(0, 0.5); tol 1e-12 (float64) / 1e-6 (float32).\n"
                    f"python scripts/bench_bcd.py --reps {args.reps} --batch {B}: HIP events around the native call, median [min, max] of "
                    f"{args.reps} calls after two warm-up calls.\nd = 8: team tier, 8 problems to a wavefront; d = 64: team tier, one problem "
                    "to a wavefront; d = 512: wave tier, 8 values per lane.\n\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
