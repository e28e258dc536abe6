"""`linear` constraint objects (lower <= A x <= upper, up to 64 rows on up to 128 coefficients): the one-wavefront kernel of
kernels_cons_linear.hip and the workgroup kernel of kernels_cons_linear_wide.hip (65 to 128 coefficients) against the route they
replace (a host visit: the numpy class through callbacks, ADELIE_HIP_CONS_HOST=1).

    python scripts/bench_cons_linear.py [n reps [wide]]

1. One binding visit through adelie_hip_cons_visit_test (HIP events around the launch) at (m, d) = (4, 4), (16, 16), (64, 64) and
   (64, 8), float64, with the objects' default settings; beside it the wall time of the host object's solve() on the same inputs
   (the numpy driver alone, without the transfers and the synchronisation a host visit adds).
2. A Gaussian path of 8 lambdas on n rows with 40 groups of 4 coefficients, every one with a linear object of 1 to 5 rows: device
   route and host route alternated in one process, `reps` runs each.
With `wide`: the visits at (m, d) = (4, 65), (16, 96), (64, 128) and (64, 65), and a path on n rows with groups of 65 / 128 / 96 / 4 /
1 / 1 coefficients whose three wide groups carry linear objects of 3 / 64 / 17 rows.
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import adelie_amd as ad  # noqa: E402
from adelie_amd import _abi, constraint  # noqa: E402


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "runs": len(v)}


def one_visit(hip, m, d, reps):
    rng = np.random.RandomState(100 + 64 * m + d)
    Q = np.asfortranarray(np.linalg.qr(rng.randn(d, d))[0])
    quad, lin0, l1, l2 = rng.uniform(0.5, 2.0, d), rng.randn(d) * 3.0, 0.5, 0.1
    A = rng.randn(m, d) / np.sqrt(d)
    w = A @ (Q @ (lin0 / (quad + l2)))
    tight = rng.rand(m) < 0.4
    tight[np.argmax(np.abs(w))] = True
    lo, up = np.where(tight & (w < 0), -0.3 * np.abs(w), -1e3), np.where(tight & (w > 0), 0.3 * np.abs(w), 1e3)
    make = lambda: constraint.linear(A, lo, up)
    x0 = 0.1 * rng.randn(d)
    beta0, grad = Q @ x0, Q @ (lin0 - quad * x0)
    cfg, va = constraint._PROX_NEWTON_DEFAULTS, make()._vars
    dev_ms, host_ms, status = [], [], 0
    for r in range(reps + 1):  # (the first of each is the warm-up)
        beta, mu, dcol, dlt = beta0.copy(), np.zeros(m), np.zeros(d, dtype=np.int32), np.zeros(d)
        order, norder = np.full(m, -1, dtype=np.int32), np.zeros(1, dtype=np.int32)
        st_f, st_i = np.zeros(4), np.zeros(5, dtype=np.int64)
        a = _abi.ConsVisit(dtype=_abi.F64, q=d, m=m, native=constraint.NATIVE_LINEAR, mark=1, first_of_pass=1, max_active_size=8,
                           l1=l1, l2=l2, dbeta_tol=0.0)
        a.cfg[:] = [cfg[k] for k in ("max_iters", "tol", "pinball_max_iters", "pinball_tol", "slack")]
        a.lin_cfg[:] = [1e5, 1e-7]
        for name, arr in (("V", Q), ("grad", grad), ("beta", beta), ("vars", quad), ("mu", mu), ("dcol", dcol), ("dlt", dlt),
                          ("st_f", st_f), ("st_i", st_i), ("lin_A", A), ("lin_lower", lo), ("lin_upper", up), ("lin_vars", va),
                          ("lin_order", order), ("lin_norder", norder)):
            setattr(a, name, arr.ctypes.data)
        hip.check(hip.fn("cons_visit_test")(C.byref(a)))
        status |= int(st_i[2])
        obj, xh = make(), beta0 @ Q
        lin = grad @ Q + quad * xh
        t0 = time.perf_counter()
        obj.solve(xh, quad, lin, l1, l2, Q)
        el = (time.perf_counter() - t0) * 1e3
        if r:
            dev_ms.append(st_f[3])
            host_ms.append(el)
    return {"m": m, "d": d, "device_kernel_ms": spread(dev_ms), "host_solve_ms": spread(host_ms), "status": status,
            "multipliers_nnz": int(np.sum(mu != 0)), "max_abs_dx_device_vs_host": float(np.abs(beta @ Q - xh).max())}


def path(n, reps, wide=False):
    sizes = np.array([65, 128, 96, 4, 1, 1] if wide else [4] * 40)
    G, p = len(sizes), int(sizes.sum())
    groups = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    rng = np.random.RandomState(3)
    X = np.asfortranarray(rng.normal(0, 1, (n, p)))
    b = rng.normal(0, 1, p) * (rng.rand(p) < 0.5)
    y = X @ b + np.sqrt(np.sum(b ** 2)) * rng.normal(0, 1, n)
    Xd = ad.matrix.dense(X)
    r = np.random.RandomState(5)
    spec = []
    for g in range(G):
        m = (3, 64, 17, 0, 0, 0)[g] if wide else r.randint(1, 6)
        scale = np.sqrt(sizes[g]) if wide else 1.0
        spec.append((r.randn(m, sizes[g]) / scale, -r.uniform(0, 0.2, m) * (r.rand(m) < 0.7), r.uniform(0.02, 0.2, m)) if m else None)
    make = lambda: [None if s is None else constraint.linear(*s) for s in spec]
    kw = dict(groups=groups, alpha=0.7, lmda_path_size=8, min_ratio=0.05, early_exit=False, progress_bar=False)
    secs, last = {"device": [], "host": []}, {}
    for rep in range(reps + 1):  # (run 0 warms both routes up)
        for arm in ("device", "host"):
            if arm == "host":
                os.environ["ADELIE_HIP_CONS_HOST"] = "1"
            try:
                t0 = time.perf_counter()
                st = ad.grpnet(Xd, ad.glm.gaussian(y), constraints=make(), **kw)  # (returns after its last synchronise)
                el = time.perf_counter() - t0
            finally:
                os.environ.pop("ADELIE_HIP_CONS_HOST", None)
            assert st.error == "", st.error
            if rep:
                secs[arm].append(el)
            last[arm] = st
    what = "groups of 65 / 128 / 96 / 4 / 1 / 1, linear objects of 3 / 64 / 17 rows on the wide ones" if wide else f"{G} groups of 4 with linear objects of 1 to 5 rows"
    out = {"workload": f"Gaussian group elastic net {n}x{p}, {what}, alpha 0.7, 8 lambdas"}
    for arm in ("device", "host"):
        c = last[arm].counters
        out[arm] = {"seconds": spread(secs[arm]), "n_dev_cons_visits": c["n_dev_cons_visits"], "n_host_cons_visits": c["n_host_cons_visits"]}
    out["max_abs_dbeta_device_vs_host"] = float(np.abs(last["device"].betas.toarray() - last["host"].betas.toarray()).max())
    return out


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    wide = len(sys.argv) > 3 and sys.argv[3] == "wide"
    hip = _abi.hip_backend()
    for m, d in ((4, 65), (16, 96), (64, 128), (64, 65)) if wide else ((4, 4), (16, 16), (64, 64), (64, 8)):
        print(json.dumps(one_visit(hip, m, d, reps)), flush=True)
    print(json.dumps(path(n, reps, wide)), flush=True)
