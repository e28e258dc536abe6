"""The per-lambda losses of a cross-validated Cox path three ways, and cv_grpnet end to end: argv [n p L folds] [--part
losses|e2e|all] [--reps R] [--out FILE] [--resources FILE].

Design and family of tests/test_gpu_cox.py::test_large_path_completes (n = 200 000, p = 5 000, f64, 3 strata), 5 folds, 100
lambdas.  Per fold the path is solved as cv._fold_loss solves it, and the losses of the same (betas, intercepts) are timed
  (a) on the host: predict + 2 L numpy losses (what cv_grpnet did for glm.cox before X.cox_path_losses existed);
  (b) as 2 L single device evaluations, glm._device_eval(eta, grad=False, hess=False), of the etas predict downloaded
      (predict's own time is reported beside it);
  (c) by X.cox_path_losses (one call).
(a) runs once per fold (its spread is the spread over the folds); (b) and (c) run `--reps` times per fold after one warm-up
call, and every time ends in a device synchronise (each route returns host numbers).  Reported: median and min..max over all
samples, the largest |a - c| / max(|a|, 1), and whether (b) and (c) are bit-equal (cv_grpnet's offsets are zero, so predict's
base + (b0 + off) and the device's (base + b0) + off are the same numbers).
End to end: wall time of cv_grpnet, `--reps` runs after one warm-up run, the device and the host route alternating in one
process (the host route by switching cv's gate off); a run in which a fold's solve logged an error stops that fold early, so
it is listed but left out of the statistics.  The script also runs on a commit without X.cox_path_losses (the host route is
what cv_grpnet takes there, and (c) is left out), so the same command gives both sides.
Appends its report to --out (default profiles/cox_cv_losses.txt); --resources names a text file (the compiler's
kernel-resource-usage remarks of the batched kernels) copied into the report."""
import json, os, sys, time, numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import adelie_amd as ad
from adelie_amd import cv as cvm


def opt(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


pos = []
it = iter(sys.argv[1:])
for a in it:
    if a.startswith("--"):
        next(it, None)
    else:
        pos.append(int(a))
n, p, L, folds = (pos + [200_000, 5_000, 100, 5][len(pos):])[:4]
part, reps = opt("--part", "all"), int(opt("--reps", "3"))
out_path = opt("--out", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "cox_cv_losses.txt"))
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def stats(xs):
    xs = np.asarray(xs, dtype=float)
    return f"median {np.median(xs):.4f} s (min {xs.min():.4f}, max {xs.max():.4f}, {len(xs)} samples)"


torch.manual_seed(0)
Xt = torch.randn(n, p, device="cuda", dtype=torch.float64).t().contiguous().t()  # column-major on the device
rng = np.random.default_rng(91)
start = np.round(rng.exponential(1, n), 1)
stop = start + np.round(rng.exponential(2, n), 1) + 0.1
status = (rng.uniform(size=n) > 0.3).astype(np.float64)
strata = rng.integers(0, 3, n)
fam = ad.glm.cox(start, stop, status, strata=strata)
Xd = ad.matrix.dense(Xt)
has_new = hasattr(Xd, "cox_path_losses") and Xd._backend.has("design_cox_path_losses")
say(f"# bench_cox_cv: n={n} p={p} f64, 3 strata, {folds} folds, {L} lambdas, reps={reps}, "
    f"X.cox_path_losses {'present' if has_new else 'absent (host route)'}; device {torch.cuda.get_device_name(0)}")
nt = (n + 1023) // 1024
say(f"Cox scratch of the batched evaluation: {(6 * n + 17 * nt) * 8} bytes per lambda (6 n + 17 ceil(n / 1024) doubles: two "
    f"families x 3 n-vectors, tile aggregates, max and loss partials); a single evaluation holds {(6 * n + 17 * nt + 1) * 8} bytes")

if part in ("losses", "all"):
    np.random.seed(0)
    order = np.random.choice(n, n, replace=False)
    ratios = np.logspace(0, -1, L)
    full_lmdas = ad.grpnet(Xd, fam, lmda_path_size=0, progress_bar=False).lmda_max * ratios
    t_solve, t_pred, t_a, t_b, t_c, worst, equal = [], [], [], [], [], 0.0, True
    for b, e in cvm.fold_ranges(n, folds):
        idx = order[b:e]
        w = fam.weights.copy()
        w[idx] = 0
        w /= np.sum(w)
        fam_c = fam.reweight(w)
        t0 = time.perf_counter()
        s0 = ad.grpnet(Xd, fam_c, lmda_path_size=0, progress_bar=False)
        curr = s0.lmda_max * ratios
        aug = np.sort(np.concatenate([full_lmdas, curr[curr > full_lmdas[0]]]))[::-1]
        s = ad.grpnet(Xd, fam_c, ddev_tol=0, early_exit=False, lmda_path=aug, progress_bar=False)
        t_solve.append(time.perf_counter() - t0)
        fb, fi = ad.diagnostic.coefficients(lmdas_new=full_lmdas, betas=s.betas, intercepts=s.intercepts, lmdas=s.lmdas)
        # (a)
        t0 = time.perf_counter()
        etas = ad.diagnostic.predict(X=Xd, betas=fb, intercepts=fi, offsets=s._offsets)
        t1 = time.perf_counter()
        a_full = np.array([fam.loss(eta) for eta in etas])
        a_train = np.array([fam_c.loss(eta) for eta in etas])
        t2 = time.perf_counter()
        t_pred.append(t1 - t0)
        t_a.append(t2 - t0)
        # (b)
        for r in range(reps + 1):
            t0 = time.perf_counter()
            b_full = np.array([fam._device_eval(eta, grad=False, hess=False)[2] for eta in etas])
            b_train = np.array([fam_c._device_eval(eta, grad=False, hess=False)[2] for eta in etas])
            if r:
                t_b.append(time.perf_counter() - t0)
        # (c)
        if has_new:
            for r in range(reps + 1):
                t0 = time.perf_counter()
                c_full, c_train = Xd.cox_path_losses(fam, fam_c, fb, fi, s._offsets)
                if r:
                    t_c.append(time.perf_counter() - t0)
            for x, y in ((a_full, c_full), (a_train, c_train)):
                worst = max(worst, float(np.max(np.abs(x - y) / np.maximum(np.abs(x), 1.0))))
            equal = equal and np.array_equal(b_full, c_full) and np.array_equal(b_train, c_train)
        del etas
        say(f"fold done: solve {t_solve[-1]:.2f} s, (a) {t_a[-1]:.2f} s of which predict {t_pred[-1]:.2f} s"
            + (f", (c) {t_c[-1]:.4f} s" if has_new else ""))
    say(f"per fold, {2 * L} losses of the same (betas, intercepts):")
    say(f"  fold path solve (both grpnet calls)        {stats(t_solve)}")
    say(f"  (a) host: predict + 2 L numpy losses       {stats(t_a)}")
    say(f"      of which predict (eta download)        {stats(t_pred)}")
    say(f"  (b) 2 L single device evaluations          {stats(t_b)}   [+ predict to have the etas on the host]")
    if has_new:
        say(f"  (c) X.cox_path_losses                      {stats(t_c)}")
        ma, mb, mc = np.median(t_a), np.median(t_b), np.median(t_c)
        say(f"  (a)/(c) = {ma / mc:.1f}x   (b)/(c) = {mb / mc:.1f}x   ((b) + predict)/(c) = {(mb + np.median(t_pred)) / mc:.1f}x")
        say(f"  largest |a - c| / max(|a|, 1) = {worst:.3e};  (b) and (c) bit-equal: {equal}")

if part in ("e2e", "all"):
    import logging

    logged = []

    class Grab(logging.Handler):
        def emit(self, rec):
            logged.append(rec.getMessage())

    logging.getLogger("adelie_amd").addHandler(Grab())
    kw = dict(n_folds=folds, lmda_path_size=L, seed=0)
    # with X.cox_path_losses the two routes alternate in one process (the host route: the gate in cv switched off)
    routes = ["device", "host"] if has_new else ["host"]
    gate = getattr(cvm, "_cox_on_device", None)
    t_e = {r: [] for r in routes}
    bad = {r: 0 for r in routes}
    ref = None
    for r in range(reps + 1):
        for route in routes:
            if has_new:
                cvm._cox_on_device = gate if route == "device" else (lambda X, glm: False)
            del logged[:]
            t0 = time.perf_counter()
            res = ad.cv_grpnet(Xd, fam, **kw)
            el = time.perf_counter() - t0
            ref = res.losses if ref is None else ref
            diff = float(np.max(np.abs(res.losses - ref) / np.maximum(np.abs(ref), 1.0)))
            say(f"  cv_grpnet run {r} ({route} losses{', warm-up' if r == 0 else ''}): {el:.3f} s, best_idx {res.best_idx}, largest "
                f"relative difference of the loss table to the first run {diff:.2e}" + (f", logged: {logged}" if logged else ""))
            if logged:   # a fold whose solve stopped with an error ends early: not a time of the same work
                bad[route] += 1
            elif r:
                t_e[route].append(el)
    if has_new:
        cvm._cox_on_device = gate
    for route in routes:
        say(f"cv_grpnet end to end, {route} losses: " + (stats(t_e[route]) if t_e[route] else "no clean run")
            + f"; runs left out because a fold's solve logged an error: {bad[route]}")

res_file = opt("--resources", None)
if res_file:
    lines.append("kernel resource usage (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):")
    lines.extend(open(res_file).read().rstrip().splitlines())
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "a") as f:
    f.write("\n".join(lines) + "\n\n")
print(json.dumps({"out": out_path, "has_new": bool(has_new)}))
