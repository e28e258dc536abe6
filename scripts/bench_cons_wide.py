"""Box / one-sided constraint objects on groups of 65 to 128 coefficients: the workgroup kernel of kernels_cons_wide.hip against
the route it replaces (a host visit: the numpy classes through callbacks, ADELIE_HIP_CONS_HOST=1).

    python scripts/bench_cons_wide.py [n reps]

1. One visit through adelie_hip_cons_visit_test (HIP events around the launch) at d = 65, 96, 128, box and one-sided, float64, on a
   problem whose bounds bind, with the objects' default settings; beside it the wall time of the host object's solve() on the same
   inputs (the numpy driver alone, without the transfers and the synchronisation a host visit adds).
2. A Gaussian path with groups of 65, 128, 96, 8, 1, 1, 1 coefficients (the first four constrained), n rows: device route and host
   route alternated in one process, `reps` runs each.
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


def one_visit(hip, native, d, reps):
    rng = np.random.RandomState(100 + d)
    Q = np.asfortranarray(np.linalg.qr(rng.randn(d, d))[0])
    quad, lin0, l1, l2 = rng.uniform(0.5, 2.0, d), rng.randn(d) * 3.0, 0.5, 0.1
    z = Q @ (lin0 / (quad + l2))
    tight = rng.rand(d) < 0.4
    if native == "box":
        va, vb = np.where(tight & (z < 0), -0.3 * np.abs(z), -1e3), np.where(tight & (z > 0), 0.3 * np.abs(z), 1e3)
        make = lambda: constraint.box(va, vb)
    else:
        va = np.where(rng.rand(d) < 0.5, -1.0, 1.0)
        vb = np.where(tight & (va * z > 0), 0.3 * np.abs(z), 1e3)
        make = lambda: constraint.one_sided(va, vb)
    x0 = 0.1 * rng.randn(d)
    beta0, grad = Q @ x0, Q @ (lin0 - quad * x0)
    cfg = constraint._PROX_NEWTON_DEFAULTS
    dev_ms, host_ms, status = [], [], 0
    for r in range(reps + 1):  # (the first of each is the warm-up)
        beta, mu, dcol, dlt = beta0.copy(), np.zeros(d), np.zeros(d, dtype=np.int32), np.zeros(d)
        st_f, st_i = np.zeros(4), np.zeros(5, dtype=np.int64)
        a = _abi.ConsVisit(dtype=_abi.F64, q=d, native=4 if native == "box" else 5, mark=1, first_of_pass=1, max_active_size=8,
                           l1=l1, l2=l2, dbeta_tol=0.0)
        a.cfg[:] = [cfg[k] for k in ("max_iters", "tol", "pinball_max_iters", "pinball_tol", "slack")]
        for name, arr in (("V", Q), ("grad", grad), ("beta", beta), ("vars", quad), ("va", va), ("vb", vb), ("mu", mu),
                          ("dcol", dcol), ("dlt", dlt), ("st_f", st_f), ("st_i", st_i)):
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
    return {"native": native, "d": d, "device_kernel_ms": spread(dev_ms), "host_solve_ms": spread(host_ms), "status": status,
            "multipliers_nnz": int(np.sum(mu != 0)), "max_abs_dx_device_vs_host": float(np.abs(beta @ Q - xh).max())}


def path(n, reps):
    sizes = np.array([65, 128, 96, 8, 1, 1, 1])
    groups = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    rng = np.random.RandomState(3)
    X = np.asfortranarray(rng.normal(0, 1, (n, 300)))
    b = rng.normal(0, 1, 300) * (rng.rand(300) < 0.5)
    y = X @ b + np.sqrt(np.sum(b ** 2)) * rng.normal(0, 1, n)
    Xd = ad.matrix.dense(X)

    def make():
        r = np.random.RandomState(5)
        return [constraint.lower(np.zeros(65)), constraint.lower(np.zeros(128)),
                constraint.box(-r.uniform(0.02, 0.2, 96), r.uniform(0.02, 0.2, 96)),
                constraint.one_sided(np.where(r.rand(8) < 0.5, -1.0, 1.0), r.uniform(0.02, 0.2, 8)), None, None, None]

    kw = dict(groups=groups, alpha=0.7, lmda_path_size=8, min_ratio=0.05, early_exit=False, progress_bar=False)
    secs, last = {"device": [], "host": []}, {}
    for r in range(reps + 1):  # (run 0 warms both routes up)
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
            if r:
                secs[arm].append(el)
            last[arm] = st
    out = {"workload": f"Gaussian group elastic net {n}x300, groups of 65/128/96/8/1/1/1, alpha 0.7, 8 lambdas"}
    for arm in ("device", "host"):
        c = last[arm].counters
        out[arm] = {"seconds": spread(secs[arm]), "n_dev_cons_visits": c["n_dev_cons_visits"], "n_host_cons_visits": c["n_host_cons_visits"]}
    out["max_abs_dbeta_device_vs_host"] = float(np.abs(last["device"].betas.toarray() - last["host"].betas.toarray()).max())
    return out


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    hip = _abi.hip_backend()
    for native in ("box", "one_sided"):
        for d in (65, 96, 128):
            print(json.dumps(one_visit(hip, native, d, reps)), flush=True)
    print(json.dumps(path(n, reps)), flush=True)
