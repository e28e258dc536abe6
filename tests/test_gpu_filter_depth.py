"""The depth rule of the filtered invariance sweep (ADELIE_HIP_FILTER_DEPTH, adelie_amd/csrc/screen_reads_host.hpp): the
sweep's threshold is put at the depth screen() is predicted to read, and screen() accepts its threshold pass iff the pivot rule
read nothing below what the pass collected.  Paths with the rule on, with the parent's rule (hook 0) and without any filtered
sweep are byte-identical; only the counts of filtered sweeps, refills and open columns differ."""
import threading

import numpy as np
import pytest

import adelie_amd as ad

pytestmark = pytest.mark.gpu

ARMS = {
    "depth": {"ADELIE_HIP_FILTER_SWEEP": "1", "ADELIE_HIP_FILTER_DEPTH": "1"},
    "need": {"ADELIE_HIP_FILTER_SWEEP": "1", "ADELIE_HIP_FILTER_DEPTH": "0"},
    "full": {"ADELIE_HIP_FILTER_SWEEP": "0", "ADELIE_HIP_FILTER_DEPTH": "1"},
}
# a 16-bit copy whatever the size of the design: the late lambdas of a small design pass the byte rule as the headline's do
SHADOW = {"ADELIE_HIP_SHADOW_KIND": "q15", "ADELIE_HIP_SHADOW_MIN_BYTES": "1"}
LASSO_SEED = 0


def make_data(n=3000, p=800, seed=LASSO_SEED, nnz=60):
    rng = np.random.RandomState(seed)
    X = np.asfortranarray(rng.normal(size=(n, p)))
    beta = np.zeros(p)
    beta[rng.choice(p, nnz, replace=False)] = rng.normal(size=nnz)
    y = X @ beta + rng.normal(size=n)
    return X, y


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def assert_identical(a, b):
    assert a.error == "" and b.error == "", (a.error, b.error)
    assert bits(a.lmdas) == bits(b.lmdas) and bits(a.intercepts) == bits(b.intercepts) and bits(a.devs) == bits(b.devs)
    A, B = a.betas.tocsr(), b.betas.tocsr()
    assert bits(A.indptr) == bits(B.indptr) and bits(A.indices) == bits(B.indices) and bits(A.data) == bits(B.data)
    assert bits(a.screen_set) == bits(b.screen_set)
    assert a.active_set_size == b.active_set_size
    assert bits(a.active_set[:a.active_set_size]) == bits(b.active_set[:b.active_set_size])
    assert bits(a.grad) == bits(b.grad) and bits(a.abs_grad) == bits(b.abs_grad) and bits(a.resid) == bits(b.resid)
    for k in ("n_basil_iters", "n_sweeps", "n_cd_visits_screen", "n_cd_visits_active", "n_new_screen_cols", "n_host_screens"):
        assert a.counters[k] == b.counters[k], (k, a.counters[k], b.counters[k])
    assert a.timers["n_screen_reads"] == b.timers["n_screen_reads"]   # (what the rule reads does not depend on the route)


def run_arm(monkeypatch, arm, solve, X, extra=None):
    for k, v in {**SHADOW, **ARMS[arm], **(extra or {})}.items():
        monkeypatch.setenv(k, v)
    return solve(ad.matrix.dense(X))


def three_arms(monkeypatch, X, solve):
    out = {arm: run_arm(monkeypatch, arm, solve, X) for arm in ARMS}
    for arm in ("depth", "need"):
        s = out[arm]
        print(arm, "filtered", s.counters["n_sweeps_filtered"], "refilled", s.counters["n_sweeps_refilled"], "of",
              s.counters["n_sweeps"], "sweeps; exact cols", s.counters["n_filter_exact_cols"], "open cols",
              int(s.timers["n_filter_open_cols"]), "reads", int(s.timers["n_screen_reads"]), "short",
              int(s.timers["n_screen_short"]))
        assert_identical(s, out["full"])
    assert out["full"].counters["n_sweeps_filtered"] == 0 and out["full"].timers["n_screen_short"] == 0
    assert out["need"].timers["n_screen_short"] == 0   # (the parent's rule predicts its own shortfalls and sweeps in full)
    return out


@pytest.fixture(scope="module")
def lasso():
    X, y = make_data()
    return X, y, dict(lmda_path_size=40, early_exit=False, tol=1e-9)


def test_lasso_filters_past_the_point_where_need_stops(hip, monkeypatch, lasso):
    """n = 3000, p = 800, 40 lambdas: 4 * need >= G within a few lambdas, after which the parent's rule filters no sweep."""
    X, y, kw = lasso
    out = three_arms(monkeypatch, X, lambda Xd: ad.grpnet(Xd, ad.glm.gaussian(y), **kw))
    assert out["need"].counters["n_sweeps_filtered"] > 0
    assert out["depth"].counters["n_sweeps_filtered"] > out["need"].counters["n_sweeps_filtered"]
    assert out["depth"].timers["n_filter_open_cols"] > 0 and out["depth"].timers["n_screen_reads"] > 0


def test_no_margin_forces_short_passes(hip, monkeypatch, lasso):
    X, y, kw = lasso
    solve = lambda Xd: ad.grpnet(Xd, ad.glm.gaussian(y), **kw)
    short = run_arm(monkeypatch, "depth", solve, X, {"ADELIE_HIP_FILTER_DEPTH_MARGIN": "0"})
    full = run_arm(monkeypatch, "full", solve, X)
    print("margin 0: short", int(short.timers["n_screen_short"]), "refilled", short.counters["n_sweeps_refilled"], "filtered",
          short.counters["n_sweeps_filtered"])
    assert short.timers["n_screen_short"] > 0
    assert_identical(short, full)


@pytest.mark.parametrize("variant", ["groups", "weights", "early_exit"])
def test_variants_are_bit_identical_across_the_three_arms(hip, monkeypatch, variant):
    X, y = make_data(n=400, p=1200, seed=3, nnz=15)
    kw = dict(lmda_path_size=30, early_exit=False, tol=1e-9)
    w = None
    if variant == "groups":
        kw.update(groups=np.arange(0, X.shape[1], 4), alpha=0.5)
    if variant == "weights":
        w = np.random.RandomState(3).uniform(0.5, 1.5, size=len(y))
        w[::4] = 0
        w /= w.sum()
    if variant == "early_exit":
        kw.update(early_exit=True)
    out = three_arms(monkeypatch, X, lambda Xd: ad.grpnet(Xd, ad.glm.gaussian(y, weights=w), **kw))
    assert out["depth"].counters["n_sweeps_filtered"] > 0


def test_warm_start(hip, monkeypatch):
    X, y = make_data(n=400, p=1200, seed=5, nnz=15)
    glm = ad.glm.gaussian(y)
    kw = dict(early_exit=False, tol=1e-9)
    monkeypatch.setenv("ADELIE_HIP_FILTER_SWEEP", "0")
    full_path = ad.grpnet(ad.matrix.dense(X), glm, lmda_path_size=30, **kw).lmdas

    def solve(Xd):
        head = ad.grpnet(Xd, glm, lmda_path=full_path[:15], **kw)
        tail = ad.grpnet(Xd, glm, lmda_path=full_path[15:], warm_start=head, **kw)
        return head, tail

    outs = {arm: run_arm(monkeypatch, arm, solve, X) for arm in ARMS}
    for arm in ("depth", "need"):
        for a, b in zip(outs[arm], outs["full"]):
            assert_identical(a, b)
    assert outs["depth"][0].counters["n_sweeps_filtered"] > 0


def test_two_concurrent_aliases(hip, monkeypatch):
    X, y = make_data(n=400, p=1200, seed=6, nnz=15)
    kw = dict(lmda_path_size=30, early_exit=False, tol=1e-9)
    full = run_arm(monkeypatch, "full", lambda Xd: ad.grpnet(Xd, ad.glm.gaussian(y), **kw), X)
    for k, v in {**SHADOW, **ARMS["depth"]}.items():
        monkeypatch.setenv(k, v)
    Xd = ad.matrix.dense(X)
    handles = [Xd, Xd.alias()]
    out = [None, None]

    def run(i):
        out[i] = ad.grpnet(handles[i], ad.glm.gaussian(y), **kw)

    ts = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    for s in out:
        assert s.counters["n_sweeps_filtered"] > 0
        assert_identical(s, full)
    assert Xd.shadow_stats()["builds"] == 1


def test_modified_adopted_tensor_retires_the_shadow_with_one_refill(hip, monkeypatch):
    import torch

    X, y = make_data(n=400, p=1200, seed=7, nnz=15)
    kw = dict(lmda_path_size=30, early_exit=False, tol=1e-9)
    for k, v in {**SHADOW, **ARMS["depth"]}.items():
        monkeypatch.setenv(k, v)
    Xt = torch.from_numpy(np.ascontiguousarray(X.T)).cuda().T
    Xd = ad.matrix.dense(Xt)
    first = ad.grpnet(Xd, ad.glm.gaussian(y), **kw)
    assert first.counters["n_sweeps_filtered"] > 0 and Xd.shadow_stats()["state"] == 1
    Xt.mul_(torch.linspace(0.5, 1.5, X.shape[1], dtype=Xt.dtype, device=Xt.device))   # every column rescaled in place
    torch.cuda.synchronize()
    on = ad.grpnet(Xd, ad.glm.gaussian(y), **kw)
    monkeypatch.setenv("ADELIE_HIP_FILTER_SWEEP", "0")
    off = ad.grpnet(Xd, ad.glm.gaussian(y), **kw)
    assert_identical(on, off)
    assert Xd.shadow_stats()["state"] == -1 and on.counters["n_sweeps_refilled"] == 1
