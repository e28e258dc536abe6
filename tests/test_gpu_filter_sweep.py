"""The filtered invariance sweep (float32 shadow of a dense f64 design, ADELIE_HIP_FILTER_SWEEP).

Kernel level (adelie_hip_filter_sweep_test against the plain full sweep of the same handle): every column marked exact carries
the bits of the full sweep, every other column lies within its bound (e_j + 4 n 2^-53 ||xs_j||) ||v|| (1 + 1e-6) of it and its
group lies below tstar * penalty in the full sweep.  Solver level: paths with the hook on and off are bit-identical."""
import threading

import numpy as np
import pytest

import adelie_amd as ad

pytestmark = pytest.mark.gpu

NEW_COUNTERS = ("n_sweeps_filtered", "n_sweeps_refilled", "n_filter_exact_cols", "n_filter_shadow_cols")


# ---- kernel level ------------------------------------------------------------------------------------------------------------
def _ptr(a):
    return a.ctypes.data if a is not None else None


def fsweep(Xd, w, r, rsum, xm, screen_groups, groups, gsizes, pen, tstar):
    p = Xd.cols()
    grad = np.empty(p)
    exact = np.zeros(p, dtype=np.uint8)
    info = np.zeros(4, dtype=np.int64)
    sg = np.ascontiguousarray(screen_groups, dtype=np.int64)
    b = Xd._backend
    b.check(b.fn("filter_sweep_test")(Xd._handle, _ptr(w), _ptr(r), float(rsum), _ptr(xm), _ptr(sg), len(sg), _ptr(groups),
                                      _ptr(gsizes), len(groups), _ptr(pen), float(tstar), _ptr(grad), _ptr(exact), _ptr(info)))
    return grad, exact.astype(bool), info


def make_problem(n, p, gs, seed, intercept=True, zero_w=True):
    rng = np.random.RandomState(seed)
    X = np.asfortranarray(rng.normal(size=(n, p)))
    w = rng.uniform(0.5, 1.5, size=n)
    if zero_w:
        w[::3] = 0.0
    w /= max(w.sum(), 1e-300)
    r = rng.normal(size=n)
    groups = np.arange(0, p, gs, dtype=np.int64)
    gsizes = np.minimum(gs, p - groups).astype(np.int64)   # (a ragged last group when gs does not divide p)
    pen = rng.uniform(0.5, 2.0, size=len(groups))
    xm = (X.T @ w) if intercept else None
    rsum = float((w * r).sum()) if intercept else 0.0
    return X, w, r, rsum, xm, groups, gsizes, pen


def bounds(X, v):
    Xs = X.astype(np.float32).astype(np.float64)
    e = np.sqrt(((X - Xs) ** 2).sum(axis=0))
    nx = np.sqrt((Xs ** 2).sum(axis=0))
    return (e + 4 * X.shape[0] * 2.0 ** -53 * nx) * np.sqrt((v ** 2).sum()) * (1 + 1e-6)


def group_norms(g, groups, gsizes):
    return np.array([np.sqrt((g[k:k + s] ** 2).sum()) for k, s in zip(groups, gsizes)])


def check_filtered(monkeypatch, Xd, X, prob, screen_groups, tstar, expect_route=True):
    _, w, r, rsum, xm, groups, gsizes, pen = prob
    monkeypatch.setenv("ADELIE_HIP_FILTER_SWEEP", "0")
    full, m_full, i_full = fsweep(Xd, w, r, rsum, xm, screen_groups, groups, gsizes, pen, tstar)
    assert i_full[2] == 0 and m_full.all()
    monkeypatch.setenv("ADELIE_HIP_FILTER_SWEEP", "1")
    got, mask, info = fsweep(Xd, w, r, rsum, xm, screen_groups, groups, gsizes, pen, tstar)
    again, mask2, info2 = fsweep(Xd, w, r, rsum, xm, screen_groups, groups, gsizes, pen, tstar)
    assert got.tobytes() == again.tobytes() and (mask == mask2).all() and (info == info2).all()   # two runs, identical bits
    assert info[2] == (1 if expect_route else 0)
    assert got[mask].tobytes() == full[mask].tobytes()
    for g in screen_groups:
        assert mask[groups[g]:groups[g] + gsizes[g]].all()
    if (~mask).any():
        bnd = bounds(X, w * r)
        d = np.abs(got - full)
        print("max |shadow - exact| / bound over the unlisted columns:", (d[~mask] / bnd[~mask]).max())
        assert (d[~mask] <= bnd[~mask]).all()
        if not info[1] & 1:   # (a list that overflowed its cap is cut off wherever the cap falls: the solver sweeps in full)
            gmask = np.array([mask[k:k + s].all() for k, s in zip(groups, gsizes)])
            assert (gmask | ~np.array([mask[k:k + s].any() for k, s in zip(groups, gsizes)])).all()   # whole groups only
            score = group_norms(full, groups, gsizes) / pen
            assert (score[~gmask] < tstar).all()
    return full, got, mask, info


@pytest.mark.parametrize("n,p,gs,intercept", [(5000, 37, 1, True), (5000, 37, 4, False), (1000, 4100, 1, True), (1000, 4100, 4, True)])
def test_filtered_sweep_against_full_sweep(hip, monkeypatch, n, p, gs, intercept):
    prob = make_problem(n, p, gs, seed=n + p + gs, intercept=intercept)
    X, w, r, rsum, xm, groups, gsizes, pen = prob
    Xd = ad.matrix.dense(X)
    G = len(groups)
    screen = list(range(0, G, 7))
    score = group_norms(X.T @ (w * r) - rsum * (xm if xm is not None else 0), groups, gsizes) / pen
    tstar = np.quantile(score, 0.9)
    _, _, mask, info = check_filtered(monkeypatch, Xd, X, prob, screen, tstar)
    assert info[1] == 0 and 0 < info[0] < p and not mask.all()
    # everything exact / nothing beyond the screen list
    _, _, mask0, info0 = check_filtered(monkeypatch, Xd, X, prob, screen, 0.0)
    scols = sum(int(gsizes[g]) for g in screen)
    if p - scols <= max(1024, p // 4):
        assert mask0.all() and info0[1] == 0
    else:   # the cap of max(1024, p/4) columns overflows: the flag tells the solver to run the full sweep
        assert info0[1] & 1 and info0[3] == p - scols and info0[0] == max(1024, p // 4)
    _, _, maski, infoi = check_filtered(monkeypatch, Xd, X, prob, screen, np.inf)
    assert infoi[0] == 0 and maski.sum() == scols
    assert Xd.shadow_stats()["builds"] == 1


def test_exact_list_sweeps_take_the_full_designs_row_splits(hip, monkeypatch):
    """n = 66000, p = 300: the full sweep splits the rows 14 ways (75 panels), a sweep shaped by a list of a dozen columns
    would split them 33 ways and sum in another order.  The listed and the screen columns must carry the full sweep's bits."""
    prob = make_problem(66000, 300, 1, seed=21)
    X, w, r, rsum, xm, groups, gsizes, pen = prob
    Xd = ad.matrix.dense(X)
    score = np.abs(X.T @ (w * r) - rsum * xm) / pen
    _, _, mask, info = check_filtered(monkeypatch, Xd, X, prob, [3, 150, 299], np.sort(score)[-9])
    assert 8 <= info[0] <= 12 and mask.sum() == info[0] + 3


def test_filtered_sweep_unaligned_and_single_row(hip, monkeypatch):
    import torch

    # an adopted column-major tensor with n = 1001: an odd leading dimension, the sweeps' unaligned path
    prob = make_problem(1001, 60, 1, seed=5)
    Xt = torch.from_numpy(np.ascontiguousarray(prob[0].T)).cuda().T
    Xd = ad.matrix.dense(Xt)
    score = np.abs(prob[0].T @ (prob[1] * prob[2]) - prob[3] * prob[4]) / prob[7]
    check_filtered(monkeypatch, Xd, prob[0], prob, [0, 11, 59], np.quantile(score, 0.8))
    # n = 1, empty screen list
    prob = make_problem(1, 9, 1, seed=6, zero_w=False)
    Xd = ad.matrix.dense(prob[0])
    check_filtered(monkeypatch, Xd, prob[0], prob, [], np.inf)
    check_filtered(monkeypatch, Xd, prob[0], prob, [], 0.0)


def test_filtered_sweep_tiny_and_unrepresentable_entries(hip, monkeypatch):
    prob = list(make_problem(2000, 40, 1, seed=9))
    X = prob[0]
    X[:, 3] *= 1e-42                      # float32 denormals: the measured e_j must still bound the column
    prob[4] = X.T @ prob[1]
    Xd = ad.matrix.dense(X)
    full, got, mask, info = check_filtered(monkeypatch, Xd, X, prob, [1], np.inf)
    assert not mask[3] and Xd.shadow_stats()["state"] == 1
    X = X.copy(order="F")
    X[0, 5] = 1e39                        # beyond FLT_MAX: the design can have no shadow, and says so
    prob[0] = X
    prob[4] = X.T @ prob[1]
    Xd = ad.matrix.dense(X)
    check_filtered(monkeypatch, Xd, X, prob, [1], np.inf, expect_route=False)
    st = Xd.shadow_stats()
    assert st["state"] == -1 and st["ineligible"] == 1 and st["builds"] == 1


# ---- solver level ------------------------------------------------------------------------------------------------------------
def make_data(n=300, p=2000, seed=0):
    rng = np.random.RandomState(seed)
    X = np.asfortranarray(rng.normal(size=(n, p)))
    beta = np.zeros(p)
    beta[rng.choice(p, 10, replace=False)] = rng.normal(size=10) * 2
    y = X @ beta + rng.normal(size=n)
    return X, y


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def assert_identical(a, b, state_too=False):
    assert a.error == "" and b.error == "", (a.error, b.error)
    assert bits(a.lmdas) == bits(b.lmdas) and bits(a.intercepts) == bits(b.intercepts) and bits(a.devs) == bits(b.devs)
    A, B = a.betas.tocsr(), b.betas.tocsr()
    assert bits(A.indptr) == bits(B.indptr) and bits(A.indices) == bits(B.indices) and bits(A.data) == bits(B.data)
    assert bits(a.screen_set) == bits(b.screen_set)
    assert a.active_set_size == b.active_set_size
    assert bits(a.active_set[:a.active_set_size]) == bits(b.active_set[:b.active_set_size])
    for k, v in b.counters.items():
        if k not in NEW_COUNTERS:
            assert a.counters[k] == v, (k, a.counters[k], v)
    if state_too:
        assert bits(a.grad) == bits(b.grad) and bits(a.abs_grad) == bits(b.abs_grad) and bits(a.resid) == bits(b.resid)


def on_off(monkeypatch, X, solve):
    """`solve(Xd)` with the hook off, then on, on fresh handles."""
    monkeypatch.setenv("ADELIE_HIP_FILTER_SWEEP", "0")
    off = solve(ad.matrix.dense(X))
    monkeypatch.setenv("ADELIE_HIP_FILTER_SWEEP", "1")
    on = solve(ad.matrix.dense(X))
    assert off.counters["n_sweeps_filtered"] == 0
    return on, off


@pytest.mark.parametrize("variant", ["lasso", "groups", "weights", "early_exit"])
def test_paths_are_bit_identical_with_the_hook_on_and_off(hip, monkeypatch, variant):
    X, y = make_data()
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
    on, off = on_off(monkeypatch, X, lambda Xd: ad.grpnet(Xd, ad.glm.gaussian(y, weights=w), **kw))
    assert_identical(on, off, state_too=True)
    print(variant, {k: on.counters[k] for k in NEW_COUNTERS}, "of", on.counters["n_sweeps"], "sweeps")
    assert on.counters["n_sweeps_filtered"] > 0


def test_warm_start_from_a_filtered_state(hip, monkeypatch):
    X, y = make_data(seed=1)
    glm = ad.glm.gaussian(y)
    kw = dict(early_exit=False, tol=1e-9)
    full_path = ad.grpnet(ad.matrix.dense(X), glm, lmda_path_size=30, **kw).lmdas

    def solve(Xd):
        head = ad.grpnet(Xd, glm, lmda_path=full_path[:15], **kw)
        tail = ad.grpnet(Xd, glm, lmda_path=full_path[15:], warm_start=head, **kw)
        return head, tail

    monkeypatch.setenv("ADELIE_HIP_FILTER_SWEEP", "0")
    head0, tail0 = solve(ad.matrix.dense(X))
    monkeypatch.setenv("ADELIE_HIP_FILTER_SWEEP", "1")
    head1, tail1 = solve(ad.matrix.dense(X))
    assert head1.counters["n_sweeps_filtered"] > 0
    assert_identical(head1, head0, state_too=True)   # ensure_exact_grad made the state's gradient exact
    assert_identical(tail1, tail0, state_too=True)


def test_alias_handles_share_the_shadow(hip, monkeypatch):
    X, y = make_data(seed=2)
    kw = dict(lmda_path_size=30, early_exit=False, tol=1e-9)
    monkeypatch.setenv("ADELIE_HIP_FILTER_SWEEP", "0")
    off = ad.grpnet(ad.matrix.dense(X), ad.glm.gaussian(y), **kw)
    monkeypatch.setenv("ADELIE_HIP_FILTER_SWEEP", "1")
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
        assert_identical(s, off, state_too=True)
    assert Xd.shadow_stats()["builds"] == 1


@pytest.mark.parametrize("drop", [False, True])
def test_modifying_an_adopted_tensor(hip, monkeypatch, drop):
    import torch

    X, y = make_data(seed=4)
    kw = dict(lmda_path_size=30, early_exit=False, tol=1e-9)
    Xt = torch.from_numpy(np.ascontiguousarray(X.T)).cuda().T
    Xd = ad.matrix.dense(Xt)
    monkeypatch.setenv("ADELIE_HIP_FILTER_SWEEP", "1")
    first = ad.grpnet(Xd, ad.glm.gaussian(y), **kw)
    assert first.counters["n_sweeps_filtered"] > 0 and Xd.shadow_stats()["state"] == 1
    Xt.mul_(torch.linspace(0.5, 1.5, X.shape[1], dtype=Xt.dtype, device=Xt.device))   # every column rescaled in place
    torch.cuda.synchronize()
    if drop:
        Xd.drop_shadow()
        assert Xd.shadow_stats()["state"] == 0
    on = ad.grpnet(Xd, ad.glm.gaussian(y), **kw)
    monkeypatch.setenv("ADELIE_HIP_FILTER_SWEEP", "0")
    off = ad.grpnet(Xd, ad.glm.gaussian(y), **kw)
    assert_identical(on, off, state_too=True)
    if drop:
        assert Xd.shadow_stats() == {"state": 1, "builds": 2, "ineligible": 0} and on.counters["n_sweeps_filtered"] > 0
    else:   # the staleness guard: the first filtered sweep finds its screen columns out of bounds and the design is retired
        assert Xd.shadow_stats()["state"] == -1 and on.counters["n_sweeps_refilled"] == 1
