"""matrix.dense on bfloat16 / float16 tensors (a design kept 16-bit in HBM, kernels_dense16.hip) on one MI355X, against the
float32 dense design of the same values.

    python scripts/bench_dense16.py [--n 100000] [--p 10000] [--sweep-reps 20] [--rounds 10] [--path-reps 3] [--out FILE]

The values are drawn on the device, so nothing of size n * p crosses the host.  Within one run:

  sweep   one full sweep (adelie_hip_bench_sweep: HIP events around --sweep-reps launches on resident buffers) in four forms --
          bf16 column-major, f16 column-major, bf16 column-major with n + 1 rows (every second column starts off a 16-byte
          boundary: what the head and tail of a column cost), the float32 dense design -- alternating over --rounds rounds:
          median and min-max, with the achieved GB/s on the bytes of the form (2 n p or 4 n p);
  path    one 100-lambda Gaussian lasso path (min_ratio 0.05, tol 1e-7, early_exit off) on the bf16 design and on the float32
          one, --path-reps repetitions each, the resident bytes of both designs and the largest difference of the coefficients.

One JSON line per part; --out also writes the text that profiles/dense16.txt holds.  No threshold and no pass mark."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import adelie_amd as ad  # noqa: E402
from adelie_amd import _abi  # noqa: E402


def sweep_ms(b, X, reps):
    ms = C.c_double()
    b.check(b.fn("bench_sweep")(X._handle, reps, C.byref(ms)))
    return ms.value


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--p", type=int, default=10000)
    ap.add_argument("--sweep-reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--path-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, p = a.n, a.p
    b = _abi.hip_backend()
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))

    gen = torch.Generator(device="cuda").manual_seed(0)

    def draw(rows, dt):  # (rows, p), column-major, values exact in dt
        return torch.randn(p, rows, device="cuda", generator=gen, dtype=torch.float32).to(dt).t()

    t_bf = draw(n, torch.bfloat16)
    forms = {
        "bf16_colmajor": (ad.matrix.dense(t_bf), n, 2),
        "f16_colmajor": (ad.matrix.dense(draw(n, torch.float16)), n, 2),
        "bf16_colmajor_n_plus_1": (ad.matrix.dense(draw(n + 1, torch.bfloat16)), n + 1, 2),
        "f32_dense": (ad.matrix.dense(t_bf.float().t().contiguous().t()), n, 4),
    }
    ms = {k: [] for k in forms}
    for X, _, _ in forms.values():
        sweep_ms(b, X, 2)  # warm-up: code objects, buffers
    for _ in range(a.rounds):
        for k, (X, _, _) in forms.items():
            ms[k].append(sweep_ms(b, X, a.sweep_reps))
    for k, (X, rows, eb) in forms.items():
        med = statistics.median(ms[k])
        emit({"part": "sweep", "form": k, "n": rows, "p": p, "rounds": a.rounds, "reps_per_round": a.sweep_reps,
              "ms_median": round(med, 4), "ms_min": round(min(ms[k]), 4), "ms_max": round(max(ms[k]), 4),
              "bytes": eb * rows * p, "GBps_at_median": round(eb * rows * p / med / 1e6, 1)})

    # one 100-lambda Gaussian lasso path on the bf16 design and on the float32 design of the same values
    Xb, Xf = forms["bf16_colmajor"][0], forms["f32_dense"][0]
    rng = np.random.default_rng(1)
    beta = np.zeros(p, np.float32)
    beta[rng.choice(p, 30, replace=False)] = rng.normal(size=30)
    y = np.zeros(n, np.float32)
    Xf.btmul(0, p, beta, y)
    y = (y + np.sqrt(30.0) * rng.normal(size=n)).astype(np.float32)
    kw = dict(lmda_path_size=100, min_ratio=0.05, tol=1e-7, early_exit=False, progress_bar=False)
    res = {}
    for name, X in (("bf16_colmajor", Xb), ("f32_dense", Xf)):
        ad.grpnet(X, ad.glm.gaussian(y, dtype=np.float32), **dict(kw, lmda_path_size=3))  # warm-up
        ts, st = [], None
        for _ in range(a.path_reps):
            t0 = time.perf_counter()
            st = ad.grpnet(X, ad.glm.gaussian(y, dtype=np.float32), **kw)
            ts.append(time.perf_counter() - t0)
            assert st.error == "", st.error
        res[name] = st
        emit({"part": "path", "design": name, "lambdas": len(st.lmdas), "s_median": round(statistics.median(ts), 4),
              "s_min": round(min(ts), 4), "s_max": round(max(ts), 4), "engine_panel": int(st.counters["engine_panel"]),
              "resident_bytes": (2 if name != "f32_dense" else 4) * n * p, "active_at_end": int((st.betas[-1] != 0).sum())})
    emit({"part": "path", "max_abs_dbeta": float(np.abs((res["bf16_colmajor"].betas - res["f32_dense"].betas)).max())})
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
