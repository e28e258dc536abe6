"""solver.pinball on one MI355X: many constraints on a modest dimension, float64, the constraint matrix generated on the device.

    python scripts/bench_pinball.py [--m 200000] [--d 512] [--pen 0.1] [--reps 2] [--cpu-m 2000] [--cpu-d 100] [--out profiles/pinball.txt]

A ~ N(0, 1) (m, d) row-major on the device; S = X'X and v = X'y of a (2 d + 8, d) Gaussian X as in tests/pinball_checks.py;
penalties pen * U(0, 1).  Prints seconds per solve (wall clock around the call: set-up, the solve and the download of the
state), iters / n_kkt / ns, the split of the solve's device time into sweeps (A resid over the m rows), AS / H builds and the fit
kernel (HIP events on the solve's stream), the fit kernel's time per changed visit (a changed visit reads one column of H,
ns * 8 bytes, and ends with one workgroup barrier), and as the CPU figure the numpy restatement of tests/pinball_checks.py (one
core) at --cpu-m x --cpu-d.  One JSON line per figure; --out writes the table that profiles/pinball.txt holds.  No pass mark:
nothing exists yet to compare these times with."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import adelie_amd as ad  # noqa: E402
import pinball_checks as pc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=200000)
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--pen", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--cpu-m", type=int, default=2000)
    ap.add_argument("--cpu-d", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    m, d = args.m, args.d
    gen = torch.Generator(device="cuda").manual_seed(0)
    At = torch.randn(m, d, dtype=torch.float64, device="cuda", generator=gen)  # (m, d) row-major: adopted in place
    _, S, v, pneg, ppos = pc.gen(1, d, 0, args.pen)
    rs = np.random.RandomState(1)
    pneg, ppos = args.pen * rs.uniform(0, 1, m), args.pen * rs.uniform(0, 1, m)
    A = ad.matrix.dense(At, method="constraint")
    ad.pinball(A, S, v, pneg, ppos, max_iters=2)  # warm-up: code objects, the device buffers
    best, state = np.inf, None
    for _ in range(args.reps):
        t0 = time.perf_counter()
        s = ad.pinball(A, S, v, pneg, ppos)
        t = time.perf_counter() - t0
        if t < best:
            best, state = t, s
    bm = state.benchmark
    ns = int(state.screen_set_size)
    dev = dict(m=m, d=d, pen=args.pen, seconds=best, solve_seconds=state.total_time, iters=state.iters, n_kkt=state.n_kkt, ns=ns,
               active=int(state.active_set_size), error=state.error, sweep_ms=bm["t_sweep_ms"], build_ms=bm["t_gram_ms"],
               fit_ms=bm["t_fit_ms"], changed_visits=int(bm["n_changed"]),
               fit_us_per_changed_visit=bm["t_fit_ms"] * 1e3 / max(bm["n_changed"], 1), h_column_bytes=ns * 8,
               sweep_gb_per_s=state.n_kkt * m * d * 8 / max(bm["t_sweep_ms"], 1e-9) / 1e6)
    print(json.dumps(dev), flush=True)
    Ac, Sc, vc, lc, uc = pc.gen(args.cpu_m, args.cpu_d, 0, args.pen)
    t0 = time.perf_counter()
    r = pc.solve(Ac, Sc, vc, lc, uc, np.float64)
    t_cpu = time.perf_counter() - t0
    t0 = time.perf_counter()
    sc = ad.pinball(Ac, Sc, vc, lc, uc)
    t_dev_small = time.perf_counter() - t0
    cpu = dict(m=args.cpu_m, d=args.cpu_d, numpy_seconds=t_cpu, device_seconds=t_dev_small, iters=r.iters, n_kkt=r.n_kkt,
               ns=len(r.screen), same_trajectory=bool(list(sc.screen_set[:sc.screen_set_size]) == r.screen and sc.iters == r.iters))
    print(json.dumps(cpu), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(f"solver.pinball on one MI355X, float64, A ~ N(0, 1) of shape ({m}, {d}) generated on the device, S = X'X of a "
                    f"({2 * d + 8}, {d}) Gaussian X, penalties {args.pen} * U(0, 1), defaults (kappa = min(m, d), tol 1e-7).\n"
                    f"scripts/bench_pinball.py, best of {args.reps} solves.\n\n"
                    f"{dev['seconds']:.3f} s per call of ad.pinball (set-up + solve + download), {dev['solve_seconds']:.3f} s inside "
                    f"adelie_hip_pinball_solve\niters {dev['iters']}, n_kkt {dev['n_kkt']}, ns {ns}, active {dev['active']}"
                    f"{', error: ' + dev['error'] if dev['error'] else ''}\n"
                    f"device time (HIP events): sweeps {dev['sweep_ms']:.2f} ms ({dev['sweep_gb_per_s']:.0f} GB/s over {dev['n_kkt']} "
                    f"full sweeps of m * d * 8 bytes), AS / H builds {dev['build_ms']:.2f} ms, fit kernel {dev['fit_ms']:.2f} ms\n"
                    f"fit kernel: {dev['changed_visits']} changed visits, {dev['fit_us_per_changed_visit']:.3f} us per changed visit "
                    f"(one column of H of ns * 8 = {ns * 8} bytes each)\n\n"
                    f"CPU figure (numpy restatement of tests/pinball_checks.py, one core) at ({args.cpu_m}, {args.cpu_d}): {t_cpu:.3f} s "
                    f"(iters {r.iters}, n_kkt {r.n_kkt}, ns {len(r.screen)}); ad.pinball on the same problem, upload included: "
                    f"{t_dev_small:.3f} s, same trajectory: {cpu['same_trajectory']}\n")


if __name__ == "__main__":
    main()
