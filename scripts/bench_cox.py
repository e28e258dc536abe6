"""Cox lasso path on the dense headline design three ways -- glm.cox (family on the device), the same family through the
host-callback route (a GlmBase64 subclass), and a binomial lasso on the same design for scale: argv n p [L] [--skip-callback].
Prints one line per run and a final JSON line: path wall time, IRLS iterations, ms per IRLS iteration, max|dbeta| between the
two Cox routes."""
import json, os, sys, time, numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import adelie_amd as ad
from bench import make_data

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n, p = int(args[0]), int(args[1]); L = int(args[2]) if len(args) > 2 else 100
X, y = make_data(n, p, 0, torch.device("cuda", 0), torch.float64)
rng = np.random.default_rng(0)
ys = (y - y.mean()) / y.std()
start = np.round(rng.exponential(1, n), 1)
stop = start + np.round(np.exp(-0.5 * ys + rng.normal(0, 1, n)), 1) + 0.1
cens = start + np.round(np.exp(rng.normal(0.5, 1, n)), 1) + 0.1
status = (stop < cens).astype(np.float64)
stop = np.minimum(stop, cens)
fam = ad.glm.cox(start, stop, status)


class CoxByCallback(ad.glm.GlmBase64):
    def __init__(self, f):
        self.f = f
        ad.glm.GlmBase64.__init__(self, "cox_cb", f.status, f.weights)

    def gradient(self, eta, grad):
        self.f.gradient(eta, grad)

    def hessian(self, eta, grad, hess):
        self.f.hessian(eta, grad, hess)

    def loss(self, eta):
        return self.f.loss(eta)

    def loss_full(self):
        return self.f.loss_full()


Xd = ad.matrix.dense(X)
out = {"n": n, "p": p, "L": L}
states = {}
runs = [("cox_device", fam), ("binomial", ad.glm.binomial((y > np.median(y)).astype(np.float64)))]
if "--skip-callback" not in sys.argv:
    runs.insert(1, ("cox_callback", CoxByCallback(fam)))
for name, g in runs:
    for rep in range(2 if name != "cox_callback" else 1):  # (the first device run includes the one-time set-up)
        t0 = time.perf_counter()
        st = ad.grpnet(Xd, g, early_exit=False, lmda_path_size=L, progress_bar=False)
        el = time.perf_counter() - t0
    it = int(st.counters["n_irls_iters"])
    states[name] = st
    out[name] = {"path_s": round(el, 3), "irls_iters": it, "ms_per_irls_iter": round(1e3 * el / max(it, 1), 3),
                 "n_solutions": len(st.lmdas), "error": st.error}
    print(name, out[name], flush=True)
if "cox_callback" in states:
    a, b = states["cox_device"], states["cox_callback"]
    m = min(len(a.lmdas), len(b.lmdas))
    out["max_abs_dbeta"] = float(np.abs(a.betas[:m].toarray() - b.betas[:m].toarray()).max())
    out["speedup_per_irls_iter"] = round(out["cox_callback"]["ms_per_irls_iter"] / out["cox_device"]["ms_per_irls_iter"], 2)
print(json.dumps(out), flush=True)
