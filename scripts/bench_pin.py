"""A pin path as one kernel launch against one launch per lambda (``state.gaussian_pin_naive``, config ``pin_path_launch``).

On one device, float64 and float32: a 100-lambda pin path (cold start, lambda from lambda_max of the restricted problem down to
1 % of it, no early exit) on screen sets of 16, 64 and 120 single coefficients and on one grouped set (24 groups of 4: 96 values)
of a dense 2000 x 256 design.  The two routes alternate in one process; each sample is one ``state.solve()``.  Two clocks per
sample: the wall time of the ``solve()`` call (marshalling, the state's set-up on the device -- Gram matrix of the screen set,
variances -- the path, the read-back), and the library's own ``total_time`` (the path and the read-back, without the set-up).
Median and min - max over the samples after a warm-up of both routes.

    python scripts/bench_pin.py [--samples 15] [--out profiles/pin_path.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import adelie_amd as ad  # noqa: E402


def problem(dtype, kind, nv, n=2000, p=256, L=100, seed=0):
    rng = np.random.default_rng(seed)
    X = np.asfortranarray(rng.normal(size=(n, p)).astype(dtype))
    q = 1 if kind == "single" else 4
    groups = np.arange(0, p, q)
    screen = rng.permutation(len(groups))[:nv // q]
    cols = np.concatenate([np.arange(groups[g], groups[g] + q) for g in screen])
    beta = np.zeros(p)
    beta[cols] = rng.normal(size=len(cols)) * (rng.uniform(size=len(cols)) < 0.5)
    y = X.astype(np.float64) @ beta + rng.normal(size=n)
    w = np.full(n, 1.0 / n)
    y_mean = float(w @ y)
    yc = y - y_mean
    y_var = float(w @ (yc * yc))
    Xc = X.astype(np.float64) - w @ X.astype(np.float64)
    g0 = Xc.T @ (w * yc)
    lmax = max(np.linalg.norm(g0[groups[g]:groups[g] + q]) for g in screen)
    lmda_path = lmax * np.exp(np.linspace(0, np.log(1e-2), L))
    design = ad.matrix.dense(X)
    return ad.state.gaussian_pin_naive(
        X=design, y_mean=y_mean, y_var=y_var, constraints=None, groups=groups, alpha=1.0, penalty=np.ones(len(groups)),
        weights=w, screen_set=screen, lmda_path=lmda_path, rsq=0.0, resid=yc, screen_beta=np.zeros(len(cols)),
        screen_is_active=np.zeros(len(screen), dtype=bool), active_set_size=0, active_set=np.zeros(len(screen), dtype=int),
        adev_tol=2, ddev_tol=-1, newton_tol=1e-12 if dtype == np.float64 else 1e-5)


def sample(state, launch):
    ad.configs.set_configs("pin_path_launch", launch)
    t0 = time.perf_counter()
    out = state.solve()
    wall = time.perf_counter() - t0
    assert out.error == "" and len(out.lmdas) == len(state.lmda_path), out.error
    assert out.counters["pin_route"] == (1 if launch else 2)
    return 1e3 * wall, 1e3 * out.total_time, out


def fmt(v):
    v = np.asarray(v)
    return f"{np.median(v):8.3f} ({v.min():.3f} - {v.max():.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["pin path, 100 lambdas, dense 2000 x 256, cold start: one launch (on) against one launch per lambda (off)",
             f"milliseconds, median (min - max) of {a.samples} alternating samples per route after a warm-up of both",
             "wall = the solve() call; lib = the library's total_time (path + read-back, without the state's set-up)", ""]
    lines.append(f"{'dtype':8s}{'screen set':22s}{'route':6s}{'wall ms':>30s}{'lib ms':>30s}{'iters':>8s}{'active':>8s}")
    try:
        for dtype in (np.float64, np.float32):
            for kind, nv in (("single", 16), ("single", 64), ("single", 120), ("grouped", 96)):
                st = problem(dtype, kind, nv)
                for launch in (True, False):
                    sample(st, launch)
                res = {True: ([], []), False: ([], [])}
                last = {}
                for _ in range(a.samples):
                    for launch in (True, False):
                        wall, lib, out = sample(st, launch)
                        res[launch][0].append(wall)
                        res[launch][1].append(lib)
                        last[launch] = out
                same = (np.array_equal(last[True].betas.data, last[False].betas.data) and
                        np.array_equal(last[True].resid, last[False].resid))
                label = f"{nv} x 1" if kind == "single" else f"{nv // 4} x 4 ({nv} values)"
                for launch in (True, False):
                    lines.append(f"{np.dtype(dtype).name:8s}{label:22s}{'on' if launch else 'off':6s}{fmt(res[launch][0]):>30s}"
                                 f"{fmt(res[launch][1]):>30s}{last[launch].iters:8d}{last[launch].active_set_size:8d}")
                r_wall = np.median(res[False][0]) / np.median(res[True][0])
                r_lib = np.median(res[False][1]) / np.median(res[True][1])
                lines.append(f"{'':36s}off / on: wall {r_wall:.2f}x, lib {r_lib:.2f}x; same bits: {same}")
    finally:
        ad.configs.set_configs("pin_path_launch", None)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
