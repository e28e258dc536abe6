"""css_cov on one MI355X: greedy and swapping, least_squares and subset_factor, float64, on a lazy_cov (the MFMA Gram, never on
the host) of a random dense design.

    python scripts/bench_css.py [--p 8192] [--k 64] [--n 16384] [--reps 3] [--cpu-p 2048] [--out profiles/css_cov.txt]

Per configuration: seconds per solve, the number of rank-one passes over the matrix (state.n_updates), and for greedy the time
of one update + score pass.  Greedy enqueues its whole loop without a host synchronisation, so the difference between a solve
with k and one with k / 2 columns is the device time of k / 2 iterations (prep, pass, arg-max); a pass reads and writes the
p x p matrix once, 2 * p^2 * 8 bytes.  The yardstick is a device-to-device copy of the same matrix in the same process, which
moves the same bytes.  The CPU figure is the numpy restatement of tests/css_checks.py (one core) at --cpu-p.
Prints one JSON line per configuration; --out writes the table that profiles/css_cov.txt holds."""
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
import css_checks as cc  # noqa: E402


def best_of(fn, reps):
    out, best = None, np.inf
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        best = min(best, time.perf_counter() - t0)
    return out, best


def copy_ms(p, reps=20):
    """Device-to-device copy of a (p, p) float64 matrix, HIP events, median of `reps`."""
    import torch

    a = torch.zeros(p * p, dtype=torch.float64, device="cuda")
    b = torch.empty_like(a)
    b.copy_(a)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--p", type=int, default=8192)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-p", type=int, default=2048)
    ap.add_argument("--cpu-k", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    p, k = args.p, args.k
    rng = np.random.default_rng(0)
    X = np.asfortranarray(rng.normal(size=(args.n, p)) / np.sqrt(args.n))
    A = ad.matrix.lazy_cov(ad.matrix.dense(X))
    del X
    bytes_pass = 2 * p * p * 8
    c_ms = copy_ms(p)
    rows = []
    for loss in ("least_squares", "subset_factor"):
        ad.css_cov(A, 2, method="greedy", loss=loss)  # warm-up: code objects, the device buffers
        g, t_g = best_of(lambda: ad.css_cov(A, k, method="greedy", loss=loss), args.reps)
        _, t_h = best_of(lambda: ad.css_cov(A, k // 2, method="greedy", loss=loss), args.reps)
        pass_ms = (t_g - t_h) / (k - k // 2) * 1e3
        rows.append(dict(method="greedy", loss=loss, p=p, k=k, seconds=t_g, passes=g.n_updates, pass_ms=pass_ms,
                         pass_GBps=bytes_pass / pass_ms / 1e6, copy_ms=c_ms, copy_GBps=bytes_pass / c_ms / 1e6,
                         pass_over_copy=pass_ms / c_ms))
        print(json.dumps(rows[-1]), flush=True)
        s, t_s = best_of(lambda: ad.css_cov(A, subset=g.subset, method="swapping", loss=loss), args.reps)
        rows.append(dict(method="swapping (from the greedy subset)", loss=loss, p=p, k=k, seconds=t_s, passes=s.n_updates,
                         attempts=s.n_attempts, swaps=s.n_swaps, error=s.error, ms_per_pass_incl_round_trips=t_s / max(s.n_updates, 1) * 1e3,
                         copy_ms=c_ms))
        print(json.dumps(rows[-1]), flush=True)
    c_ms2 = copy_ms(p)
    # the CPU figure: the numpy restatement, one core
    S = cc.wishart(args.cpu_p, 0)
    cpu = []
    for loss in ("least_squares", "subset_factor"):
        t0 = time.perf_counter()
        r = cc.greedy(S, args.cpu_k, loss, np.float64)
        t = time.perf_counter() - t0
        cpu.append(dict(method="numpy greedy", loss=loss, p=args.cpu_p, k=args.cpu_k, seconds=t, passes=r.n_updates,
                        pass_ms=t / max(r.n_updates, 1) * 1e3))
        print(json.dumps(cpu[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(f"css_cov on one MI355X, float64, lazy_cov of a random dense ({args.n}, {p}) design, k = {k}.  scripts/bench_css.py,\n"
                    f"best of {args.reps} solves (wall clock around the call, which ends with the solve's one synchronisation).\n"
                    f"A pass = S_resid += c beta beta^T fused with the scores of all columns: reads and writes p^2 values, "
                    f"{bytes_pass / 1e6:.0f} MB.\n"
                    f"Device-to-device copy of the same matrix (same bytes), HIP events, median of 20: {c_ms:.4f} ms before, "
                    f"{c_ms2:.4f} ms after = {bytes_pass / c_ms / 1e6:.0f} GB/s.\n\n")
            for r in rows:
                if r["method"] == "greedy":
                    f.write(f"greedy   {r['loss']:14s} {r['seconds']:.4f} s per solve, {r['passes']} passes; one iteration (prep + pass + "
                            f"arg-max, from the k = {k} and k = {k // 2} solves) {r['pass_ms']:.4f} ms = {r['pass_GBps']:.0f} GB/s "
                            f"= {r['pass_over_copy']:.2f}x the copy\n")
                else:
                    f.write(f"swapping {r['loss']:14s} {r['seconds']:.4f} s per solve, {r['passes']} passes, {r['attempts']} attempts "
                            f"(one host round trip each), {r['swaps']} swaps; {r['ms_per_pass_incl_round_trips']:.4f} ms per pass "
                            f"including the round trips{'; error: ' + r['error'] if r['error'] else ''}\n")
            f.write("\nCPU figure (numpy restatement of tests/css_checks.py, one core):\n")
            for r in cpu:
                f.write(f"numpy greedy {r['loss']:14s} p = {r['p']}, k = {r['k']}: {r['seconds']:.3f} s, {r['pass_ms']:.1f} ms per "
                        f"update + score pass ({2 * r['p'] ** 2 * 8 / r['pass_ms'] / 1e6:.1f} GB/s at 2 p^2 8 bytes)\n")


if __name__ == "__main__":
    main()
