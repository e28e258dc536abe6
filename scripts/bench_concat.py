"""matrix.concatenate(..., axis=1, resident="pieces") on one MI355X, float64: a few dense covariates in front of a large 2-bit
block (the GWAS design), kept as pieces against the dense copy that resident="auto" makes of the same pieces.

    python scripts/bench_concat.py [--n 500000] [--p 20000] [--q 16] [--sweep-reps 20] [--rounds 5] [--path-reps 3] [--out FILE]

The 2-bit calls are drawn on the device (about 5 % missing, the column means as impute values) and packed in place, the
covariates are a resident tensor adopted in place, so nothing of size n * p crosses the host.  Within one run:

  bytes   resident bytes of the pieces design (the 2-bit block n * p / 4 with its column padding and impute values, the
          covariates n * q * 8, nothing for the design itself) against the dense copy (padded n * (p + q) * 8);
  sweep   one full sweep (adelie_hip_bench_sweep: HIP events around --sweep-reps launches on resident buffers) on the pieces
          design, on the two pieces swept separately with their own kernels, and on the dense copy, alternating over --rounds
          rounds, every round listed;
  path    one 50-lambda Gaussian lasso path (min_ratio 0.05, tol 1e-7, early_exit off; the covariates unpenalised) on the pieces
          design and on the dense copy, --path-reps repetitions each with the run-to-run spread, and the largest difference
          between the two routes' coefficients.

One JSON line per part; --out also writes the text that profiles/concat_pieces.txt holds.  No threshold and no pass mark: the
pieces design buys memory and reach, and the figures say what it costs."""
import argparse
import ctypes as C
import gc
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import adelie_amd as ad  # noqa: E402
from adelie_amd import _abi  # noqa: E402


def owned(b):
    gc.collect()
    return int(b.fn("design_owned_bytes")())


def sweep_ms(b, X, reps):
    ms = C.c_double()
    b.check(b.fn("bench_sweep")(X._handle, reps, C.byref(ms)))
    return ms.value


def spread(ts):
    return (max(ts) - min(ts)) / min(ts)


def run_paths(X, glm, pen, reps):
    kw = dict(lmda_path_size=50, min_ratio=0.05, tol=1e-7, early_exit=False, progress_bar=False, penalty=pen)
    ad.grpnet(X, glm, **dict(kw, lmda_path_size=3))  # warm-up: code objects, the device buffers
    times, st = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        st = ad.grpnet(X, glm, **kw)
        times.append(time.perf_counter() - t0)
        assert st.error == "", st.error
    return times, st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=500000)
    ap.add_argument("--p", type=int, default=20000)
    ap.add_argument("--q", type=int, default=16)
    ap.add_argument("--sweep-reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--path-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    n, p, q = args.n, args.p, args.q
    b = _abi.hip_backend()
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)

    # ---- the pieces -------------------------------------------------------------------------------------------------------
    base = owned(b)
    cov_t = torch.randn(q, n, device=dev, dtype=torch.float64, generator=gen).t()      # (n, q), strides (1, n)
    calls_t = torch.empty(p, n, device=dev, dtype=torch.int8)
    chunk = max(1, (1 << 28) // n)
    for c0 in range(0, p, chunk):
        c1 = min(p, c0 + chunk)
        u = torch.rand(c1 - c0, n, device=dev, generator=gen)
        maf = 0.05 + 0.45 * torch.rand(c1 - c0, 1, device=dev, generator=gen)
        g = (u < maf * maf).to(torch.int8) + (u < maf * (2 - maf)).to(torch.int8)      # Hardy-Weinberg counts 0 / 1 / 2
        miss = torch.rand(c1 - c0, n, device=dev, generator=gen) < 0.05
        calls_t[c0:c1] = torch.where(miss, torch.full_like(g, -9), g)
        del u, g, miss
    D = ad.matrix.dense(cov_t)
    S = ad.matrix.snp_calldata(calls_t.t())
    del calls_t
    torch.cuda.empty_cache()
    snp_bytes = owned(b) - base
    cov_bytes = n * q * 8                                                                 # (adopted: the tensor's own memory)
    X = ad.matrix.concatenate([D, S], axis=1, resident="pieces")
    pieces_extra = owned(b) - base - snp_bytes
    t0 = time.perf_counter()
    Xd = ad.matrix.concatenate([D, S], axis=1)
    torch.cuda.synchronize()
    copy_s = time.perf_counter() - t0
    dense_bytes = owned(b) - base - snp_bytes - pieces_extra
    rows = [dict(part="bytes", n=n, p=p, q=q, snp_piece_bytes=snp_bytes, dense_piece_bytes=cov_bytes, pieces_design_bytes=pieces_extra,
                 pieces_total_bytes=snp_bytes + cov_bytes + pieces_extra, dense_copy_bytes=dense_bytes,
                 arithmetic_pieces_bytes=n * p // 4 + n * q * 8, arithmetic_dense_bytes=n * (p + q) * 8,
                 ratio=dense_bytes / (snp_bytes + cov_bytes + pieces_extra), dense_copy_build_s=copy_s)]
    print(json.dumps(rows[-1]), flush=True)

    # ---- one full sweep ---------------------------------------------------------------------------------------------------
    for M in (X, D, S, Xd):
        sweep_ms(b, M, 2)
    t = {"pieces": [], "dense_piece": [], "snp_piece": [], "dense_copy": []}
    for _ in range(args.rounds):
        t["pieces"].append(sweep_ms(b, X, args.sweep_reps))
        t["dense_piece"].append(sweep_ms(b, D, args.sweep_reps))
        t["snp_piece"].append(sweep_ms(b, S, args.sweep_reps))
        t["dense_copy"].append(sweep_ms(b, Xd, args.sweep_reps))
    med = {k: float(np.median(v)) for k, v in t.items()}
    rows.append(dict(part="sweep", reps=args.sweep_reps, rounds=args.rounds, pieces_ms=med["pieces"], dense_piece_ms=med["dense_piece"],
                     snp_piece_ms=med["snp_piece"], sum_of_pieces_ms=med["dense_piece"] + med["snp_piece"], dense_copy_ms=med["dense_copy"],
                     pieces_over_sum=med["pieces"] / (med["dense_piece"] + med["snp_piece"]),
                     dense_copy_over_pieces=med["dense_copy"] / med["pieces"], all_ms=t))
    print(json.dumps(rows[-1]), flush=True)

    # ---- one 50-lambda Gaussian lasso path ----------------------------------------------------------------------------------
    rs = np.random.RandomState(2)
    beta = np.zeros(p + q)
    beta[:q] = rs.normal(size=q) * 0.5
    beta[q + rs.choice(p, 40, replace=False)] = rs.choice([-1.0, 1.0], 40) * rs.uniform(0.3, 0.8, 40)
    eta = np.asarray(X @ beta)
    y = eta + np.sqrt(np.var(eta)) * rs.normal(size=n)
    glm = ad.glm.gaussian(y)
    pen = np.ones(p + q)
    pen[:q] = 0.0
    tp, sp_ = run_paths(X, glm, pen, args.path_reps)
    td, sd = run_paths(Xd, glm, pen, args.path_reps)
    dbeta = float(abs(sp_.betas - sd.betas).max())
    rows.append(dict(part="path", lambdas=50, reps=args.path_reps, pieces_s=tp, dense_copy_s=td, pieces_best_s=min(tp), dense_copy_best_s=min(td),
                     pieces_spread=spread(tp), dense_copy_spread=spread(td), pieces_over_dense_copy=min(tp) / min(td),
                     final_active=int(sp_.active_set_size), final_active_dense_copy=int(sd.active_set_size), max_abs_dbeta=dbeta,
                     pieces_engine_panel=int(sp_.counters["engine_panel"]), dense_copy_engine_panel=int(sd.counters["engine_panel"]),
                     pieces_n_sweeps=int(sp_.counters["n_sweeps"]), dense_copy_n_sweeps=int(sd.counters["n_sweeps"]),
                     pieces_sweep_ms=sp_.timers["t_sweep_ms"], dense_copy_sweep_ms=sd.timers["t_sweep_ms"],
                     pieces_gram_ms=sp_.timers["t_gram_ms"], dense_copy_gram_ms=sd.timers["t_gram_ms"]))
    print(json.dumps(rows[-1]), flush=True)

    if args.out:
        by, sw, pa = rows
        gb = 1e9
        with open(args.out, "w") as f:
            f.write("matrix.concatenate(..., axis=1, resident=\"pieces\") on one MI355X, float64 (scripts/bench_concat.py): "
                    f"{q} dense covariates in front\nof a 2-bit block of {n} x {p}, kept as pieces, against the dense copy "
                    "resident=\"auto\" makes of the same pieces.\n\n")
            f.write("Resident bytes (adelie_hip_design_owned_bytes; the adopted covariates are the tensor's own n * q * 8)\n"
                    f"  pieces design   {by['pieces_total_bytes'] / gb:.3f} GB = 2-bit piece {by['snp_piece_bytes'] / gb:.3f} GB + dense piece "
                    f"{by['dense_piece_bytes'] / gb:.3f} GB + the design itself {by['pieces_design_bytes']} bytes   "
                    f"(n p / 4 + n q 8 = {by['arithmetic_pieces_bytes'] / gb:.3f} GB)\n"
                    f"  dense copy      {by['dense_copy_bytes'] / gb:.3f} GB   (n (p + q) 8 = {by['arithmetic_dense_bytes'] / gb:.3f} GB), "
                    f"built in {by['dense_copy_build_s']:.2f} s   ratio {by['ratio']:.1f}\n\n")
            f.write(f"One full sweep (adelie_hip_bench_sweep, HIP events, median of {sw['rounds']} alternating rounds of {sw['reps']} launches)\n"
                    f"  pieces design   {sw['pieces_ms']:.3f} ms   rounds {[round(x, 3) for x in sw['all_ms']['pieces']]}\n"
                    f"  2-bit piece     {sw['snp_piece_ms']:.3f} ms   rounds {[round(x, 3) for x in sw['all_ms']['snp_piece']]}\n"
                    f"  dense piece     {sw['dense_piece_ms']:.3f} ms   rounds {[round(x, 3) for x in sw['all_ms']['dense_piece']]}\n"
                    f"  sum of pieces   {sw['sum_of_pieces_ms']:.3f} ms   pieces design / sum = {sw['pieces_over_sum']:.3f}\n"
                    f"  dense copy      {sw['dense_copy_ms']:.3f} ms   rounds {[round(x, 3) for x in sw['all_ms']['dense_copy']]}   "
                    f"dense copy / pieces design = {sw['dense_copy_over_pieces']:.2f}\n\n")
            f.write(f"One 50-lambda Gaussian lasso path (covariates unpenalised, min_ratio 0.05, tol 1e-7; wall clock of ad.grpnet, {pa['reps']} repetitions)\n"
                    f"  pieces design   {[round(x, 3) for x in pa['pieces_s']]} s   best {pa['pieces_best_s']:.3f} s   spread {100 * pa['pieces_spread']:.1f} %   "
                    f"engine_panel {pa['pieces_engine_panel']}   sweeps {pa['pieces_n_sweeps']} in {pa['pieces_sweep_ms']:.1f} ms   Gram {pa['pieces_gram_ms']:.1f} ms\n"
                    f"  dense copy      {[round(x, 3) for x in pa['dense_copy_s']]} s   best {pa['dense_copy_best_s']:.3f} s   spread {100 * pa['dense_copy_spread']:.1f} %   "
                    f"engine_panel {pa['dense_copy_engine_panel']}   sweeps {pa['dense_copy_n_sweeps']} in {pa['dense_copy_sweep_ms']:.1f} ms   Gram {pa['dense_copy_gram_ms']:.1f} ms\n"
                    f"  pieces / dense copy = {pa['pieces_over_dense_copy']:.2f}   final active set {pa['final_active']} / {pa['final_active_dense_copy']}   "
                    f"max |beta_pieces - beta_dense| = {pa['max_abs_dbeta']:.2e}\n\n")
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
