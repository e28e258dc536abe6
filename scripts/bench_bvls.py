"""solver.bvls on one MI355X: a Gaussian problem in [-0.5, 1.5] bounds, float64, the design generated on the device.

    python scripts/bench_bvls.py [--n 100000] [--p 10000] [--reps 2] [--cpu-n 2000] [--cpu-p 500] [--out profiles/bvls.txt]

X ~ N(0, 1), y = X (2 N(0, 1)) + N(0, 1).  Prints seconds per solve (wall clock around the call: set-up products, the solve and
the download of the state), iters / n_kkt / ns, the split of the solve's device time into sweeps (w * r and X^T of it), Gram
builds and the fit kernel (HIP events on the solve's stream), the fit kernel's time per changed visit (a changed visit reads
one Gram column, ns * 8 bytes, and ends with one workgroup barrier), and as the CPU figure the numpy restatement of
tests/bvls_checks.py (one core) at --cpu-n x --cpu-p.  One JSON line per figure; --out writes the table that profiles/bvls.txt
holds.  No pass mark: nothing exists yet to compare these times with."""
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
import bvls_checks as bc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--p", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--cpu-n", type=int, default=2000)
    ap.add_argument("--cpu-p", type=int, default=500)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    n, p = args.n, args.p
    gen = torch.Generator(device="cuda").manual_seed(0)
    Xt = torch.randn(p, n, dtype=torch.float64, device="cuda", generator=gen).T  # (n, p), column-major
    coef = 2 * torch.randn(p, dtype=torch.float64, device="cuda", generator=gen)
    y = (Xt @ coef + torch.randn(n, dtype=torch.float64, device="cuda", generator=gen)).cpu().numpy()
    X = ad.matrix.dense(Xt)
    lower, upper = np.full(p, -0.5), np.full(p, 1.5)
    ad.bvls(X, y, lower, upper, max_iters=2)  # warm-up: code objects, the device buffers
    best, state = np.inf, None
    for _ in range(args.reps):
        t0 = time.perf_counter()
        s = ad.bvls(X, y, lower, upper)
        t = time.perf_counter() - t0
        if t < best:
            best, state = t, s
    bm = state.benchmark
    ns = int(state.screen_set_size)
    dev = dict(n=n, p=p, seconds=best, solve_seconds=state.total_time, iters=state.iters, n_kkt=state.n_kkt, ns=ns,
               active=int(state.active_set_size), error=state.error, sweep_ms=bm["t_sweep_ms"], gram_ms=bm["t_gram_ms"],
               fit_ms=bm["t_fit_ms"], changed_visits=int(bm["n_changed"]),
               fit_us_per_changed_visit=bm["t_fit_ms"] * 1e3 / max(bm["n_changed"], 1), gram_column_bytes=ns * 8)
    print(json.dumps(dev), flush=True)
    Xc, yc, lc, uc = bc.gaussian(args.cpu_n, args.cpu_p, 0)
    t0 = time.perf_counter()
    r = bc.solve(Xc, yc, lc, uc, np.float64)
    t_cpu = time.perf_counter() - t0
    t0 = time.perf_counter()
    sc = ad.bvls(Xc, yc, lc, uc)
    t_dev_small = time.perf_counter() - t0
    cpu = dict(n=args.cpu_n, p=args.cpu_p, numpy_seconds=t_cpu, device_seconds=t_dev_small, iters=r.iters, n_kkt=r.n_kkt,
               ns=len(r.screen), same_trajectory=bool(list(sc.screen_set[:sc.screen_set_size]) == r.screen and sc.iters == r.iters))
    print(json.dumps(cpu), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(f"solver.bvls on one MI355X, float64, X ~ N(0, 1) of shape ({n}, {p}) generated on the device, bounds [-0.5, 1.5], "
                    f"defaults (kappa = min(n, p), tol 1e-7).\nscripts/bench_bvls.py, best of {args.reps} solves.\n\n"
                    f"{dev['seconds']:.3f} s per call of ad.bvls (set-up products + solve + download), {dev['solve_seconds']:.3f} s inside "
                    f"adelie_hip_bvls_solve\niters {dev['iters']}, n_kkt {dev['n_kkt']}, ns {ns}, active {dev['active']}"
                    f"{', error: ' + dev['error'] if dev['error'] else ''}\n"
                    f"device time (HIP events): sweeps {dev['sweep_ms']:.2f} ms, Gram builds {dev['gram_ms']:.2f} ms, fit kernel "
                    f"{dev['fit_ms']:.2f} ms\nfit kernel: {dev['changed_visits']} changed visits, "
                    f"{dev['fit_us_per_changed_visit']:.3f} us per changed visit (one Gram column of ns * 8 = {ns * 8} bytes each)\n\n"
                    f"CPU figure (numpy restatement of tests/bvls_checks.py, one core) at ({args.cpu_n}, {args.cpu_p}): {t_cpu:.3f} s "
                    f"(iters {r.iters}, n_kkt {r.n_kkt}, ns {len(r.screen)}); ad.bvls on the same problem, upload included: "
                    f"{t_dev_small:.3f} s, same trajectory: {cpu['same_trajectory']}\n")


if __name__ == "__main__":
    main()
