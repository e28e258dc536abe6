"""``state.gaussian_pin_naive`` / ``state.gaussian_pin_cov`` on the device: block coordinate descent along a given lambda path on
a screen set that never changes, as one kernel launch (``kernels_cd_pin.hip``), as one launch per lambda, and on the block /
panel engines.

Checked against the CPU restatement of the reference on the design restricted to the screen set, against the KKT conditions
from first principles, route against route bit for bit, and on the reference's own continuation test
(``tests/test_solver.py:516-532`` upstream).  Tolerances: the project's path tolerances (1e-6 in float64, 1e-3 in float32).

Choices of this file that its checks depend on:

* float32 runs pass ``newton_tol=1e-5`` to the pin state and to the reference alike (1e-12 is below float32 resolution);
* ``resid`` is the reference's attribute, ``y_c - X beta`` on the uncentred design; the identities about the centred residual
  ``y_c - X_c beta`` (``rsq`` among them) are asserted on ``resid - resid_sum``, which is that vector when there is an intercept;
* the continuation steps to ``0.8 * lmdas[-1]`` and is compared with row 5 of a 6-lambda solve whose last lambda is that number;
* the 160- and 300-column problems scale ``y`` to ``y_var = 1``, so that the reference's tolerance ``tol * y_var`` is the pin
  state's absolute ``tol``; the 160-column one runs on a design kept sparse, the only fixed-weight route to the block engine."""
import functools
import logging

import numpy as np
import pytest
from scipy.sparse import csc_matrix

import adelie_amd as ad
from util import kkt_gaussian

pytestmark = pytest.mark.gpu

N, P, L = 60, 24, 6
LASSO_SCREEN = [17, 3, 21, 8, 0, 12, 5, 23, 10]          # 9 groups of one, not ascending
GROUP_SIZES = [1, 3, 4, 1, 3, 4, 1, 3, 4]                # sums to 24
GROUP_SCREEN = [2, 0, 7, 4, 5]                           # sizes 4, 1, 3, 3, 4


def _atol(dtype):
    return 1e-6 if dtype == np.float64 else 1e-3


def _newton(dtype):
    """(the default newton_tol = 1e-12 is below float32 resolution: the reference's Newton root find then reports its
    iteration limit, and so does every engine here; 1e-5 is what the project's float32 group tests pass)"""
    return dict(newton_tol=1e-12 if dtype == np.float64 else 1e-5)


def _problem(kind, dtype, intercept, alpha, seed=0, n=N, p=P, screen=None, n_lmda=L, unit_var=False):
    """Data, the cold pin start on it and the lambda path 0.8 * lmda_max(restricted) * 0.7^l."""
    rng = np.random.default_rng(seed)
    X = np.asfortranarray(rng.normal(size=(n, p)).astype(dtype))
    if kind == "lasso":
        sizes = np.ones(p, dtype=int)
        screen = np.array(LASSO_SCREEN if screen is None else screen)
    else:
        sizes = np.array(GROUP_SIZES)
        screen = np.array(GROUP_SCREEN)
    groups = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(int)
    w = rng.uniform(0.5, 1.5, n)
    w = (w / w.sum()).astype(dtype)
    penalty = rng.uniform(0.5, 1.5, len(groups)).astype(dtype)
    cols = np.concatenate([np.arange(groups[g], groups[g] + sizes[g]) for g in screen])
    beta = np.zeros(p)
    beta[cols] = rng.normal(size=len(cols)) * (rng.uniform(size=len(cols)) < 0.7)
    y = X.astype(np.float64) @ beta + 0.5 * rng.normal(size=n) + 0.3
    if unit_var:  # y_var = 1: the reference's tolerance tol * y_var and the pin state's absolute tol are then the same number
        y = y / np.sqrt(np.sum(w.astype(np.float64) * (y - np.sum(w.astype(np.float64) * y)) ** 2))
    y = y.astype(dtype)
    y64, w64, X64 = y.astype(np.float64), w.astype(np.float64), X.astype(np.float64)
    y_mean = float(np.sum(w64 * y64)) if intercept else 0.0
    yc = y64 - y_mean
    y_var = float(np.sum(w64 * yc * yc))
    Xc = X64 - (w64 @ X64 if intercept else 0.0)
    g0 = Xc.T @ (w64 * yc)
    lmax = max(np.linalg.norm(g0[groups[g]:groups[g] + sizes[g]]) / penalty[g] for g in screen) / max(alpha, 1e-3)
    lmda_path = (0.8 * lmax * 0.7 ** np.arange(n_lmda)).astype(dtype)
    return dict(X=X, y=y, w=w, groups=groups, sizes=sizes, penalty=penalty, screen=screen, cols=cols, y_mean=y_mean, y_var=y_var,
                yc=yc, Xc=Xc, lmda_path=lmda_path, alpha=alpha, intercept=intercept, dtype=dtype, kind=kind)


def _cold(d, design=None, lmda_path=None, **kw):
    nv = int(np.sum(d["sizes"][d["screen"]]))
    args = dict(
        X=design if design is not None else ad.matrix.dense(d["X"]), y_mean=d["y_mean"], y_var=d["y_var"],
        constraints=None, groups=d["groups"], alpha=d["alpha"], penalty=d["penalty"], weights=d["w"], screen_set=d["screen"],
        lmda_path=d["lmda_path"] if lmda_path is None else lmda_path, rsq=0.0, resid=d["yc"].astype(d["dtype"]),
        screen_beta=np.zeros(nv), screen_is_active=np.zeros(len(d["screen"]), dtype=bool), active_set_size=0,
        active_set=np.zeros(len(d["screen"]), dtype=int), intercept=d["intercept"], tol=1e-12, adev_tol=2, ddev_tol=-1,
        **_newton(d["dtype"]))
    args.update(kw)
    return ad.state.gaussian_pin_naive(**args)


def _solve(state, launch):
    ad.configs.set_configs("pin_path_launch", launch)
    try:
        return state.solve()
    finally:
        ad.configs.set_configs("pin_path_launch", None)


def _same_bits(a, b, rows=None, cov=False):
    """The attributes the two routes must agree on bit for bit (`rows`: only the path, and only its first rows)."""
    sl = slice(None) if rows is None else slice(0, rows)
    A, B = a.betas[sl], b.betas[sl]
    for x, y in ((A.data, B.data), (A.indices, B.indices), (A.indptr, B.indptr), (a.intercepts[sl], b.intercepts[sl]),
                 (a.rsqs[sl], b.rsqs[sl]), (a.lmdas[sl], b.lmdas[sl])):
        assert np.array_equal(np.asarray(x), np.asarray(y))
    if rows is not None:
        return
    assert a.active_set_size == b.active_set_size and a.iters == b.iters and a.rsq == b.rsq
    assert np.array_equal(a.screen_beta, b.screen_beta) and np.array_equal(a.screen_is_active, b.screen_is_active)
    assert np.array_equal(a.active_set[:a.active_set_size], b.active_set[:b.active_set_size])
    if cov:
        assert np.array_equal(a.screen_grad, b.screen_grad)
    else:
        assert np.array_equal(a.resid, b.resid) and a.resid_sum == b.resid_sum


CASES = [(k, dt, ic, al) for k in ("lasso", "group") for dt in (np.float64, np.float32) for ic in (True, False) for al in (1.0, 0.6)]
_ids = lambda c: f"{c[0]}-{np.dtype(c[1]).name}-{'icpt' if c[2] else 'noicpt'}-a{c[3]}"


@functools.lru_cache(maxsize=None)
def _case(kind, dtype, intercept, alpha):
    """One problem, solved once per route (shared by the tests below, never modified)."""
    d = _problem(kind, dtype, intercept, alpha)
    st = _cold(d)
    return d, st, _solve(st, True), _solve(st, False)


@functools.lru_cache(maxsize=None)
def _reference(kind, dtype, intercept, alpha):
    """The same problem on the design restricted to the screen set, solved by the CPU restatement of the reference."""
    from oracle import oracle as orc

    orc.build()
    d = _problem(kind, dtype, intercept, alpha)
    order = np.sort(d["screen"])
    cols = np.concatenate([np.arange(d["groups"][g], d["groups"][g] + d["sizes"][g]) for g in order])
    sizes = d["sizes"][order]
    rgroups = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(int)
    ref = ad.grpnet(orc.dense(np.asfortranarray(d["X"][:, cols])), ad.glm.gaussian(d["y"], weights=d["w"]), groups=rgroups,
                    penalty=d["penalty"][order], alpha=alpha, intercept=intercept, lmda_path=d["lmda_path"], early_exit=False,
                    tol=1e-12, progress_bar=False, **_newton(dtype))
    assert ref.error == ""
    B = np.zeros((len(ref.lmdas), d["X"].shape[1]))
    B[:, cols] = ref.betas.toarray()
    return B, np.asarray(ref.intercepts, dtype=np.float64), np.asarray(ref.devs, dtype=np.float64) * d["y_var"]


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_cold_pin_path_matches_reference_on_restricted_design(hip, case):
    d, st, on, _ = _case(*case)
    B, icpt, rsqs = _reference(*case)
    tol = _atol(case[1])
    assert on.error == "" and on.betas.shape == (L, P) and len(on.lmdas) == L
    assert np.abs(on.betas.toarray() - B).max() <= tol
    assert np.abs(on.intercepts - icpt).max() <= tol
    assert np.abs(on.rsqs - rsqs).max() <= tol * d["y_var"]
    outside = np.setdiff1d(np.arange(P), d["cols"])
    assert not np.isin(on.betas.indices, outside).any()          # not stored, hence exactly zero
    assert on.counters["pin_route"] == 1
    assert on.check(method="assert")
    # the original state is left untouched
    assert st.betas.shape[0] == 0 and st.active_set_size == 0 and not st.screen_beta.any()


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_kkt_and_invariants_from_first_principles(hip, case):
    d, _, on, _ = _case(*case)
    f64 = case[1] == np.float64
    # the restricted problem: groups outside the screen set carry no condition, so give them an infinite penalty
    pen = np.full(len(d["groups"]), np.inf)
    pen[d["screen"]] = d["penalty"][d["screen"]]
    worst = kkt_gaussian(d["X"].astype(np.float64), d["y"].astype(np.float64), d["w"].astype(np.float64), d["groups"], d["sizes"],
                         pen, d["alpha"], d["intercept"], on.betas, on.intercepts, on.lmdas, 0)
    assert worst < (5e-7 if f64 else 1e-3), worst
    beta = on.betas[-1].toarray().ravel().astype(np.float64)
    w = d["w"].astype(np.float64)
    bound = (1e-12 if f64 else 1e-4) * d["y_var"]
    # `resid` is the reference's attribute, y_c - X beta on the UNcentred design (state.py:502-503 upstream); with an intercept
    # the centred residual y_c - X_c beta is resid - resid_sum (the weights sum to 1), and that is the one rsq is about
    assert np.abs(on.resid - (d["yc"] - d["X"].astype(np.float64) @ beta)).max() <= bound
    assert abs(on.resid_sum - np.sum(w * on.resid.astype(np.float64))) <= bound
    centred = d["yc"] - d["Xc"] @ beta
    mine = on.resid.astype(np.float64) - (float(on.resid_sum) if d["intercept"] else 0.0)
    assert np.abs(mine - centred).max() <= bound
    assert abs(on.rsq - (np.sum(w * d["yc"] ** 2) - np.sum(w * mine ** 2))) <= bound


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_one_launch_and_one_launch_per_lambda_give_the_same_bits(hip, case):
    _, st, on, off = _case(*case)
    assert on.error == "" and off.error == ""
    _same_bits(on, off)
    _same_bits(on, _solve(st, True))
    assert on.counters["pin_route"] == 1 and on.counters["n_pin_launches"] == 1
    assert off.counters["pin_route"] == 2 and off.counters["n_pin_launches"] == len(off.lmdas) == L


@pytest.mark.parametrize("screen,n_lmda", [([7], L), ([7], 1)], ids=["one-group", "one-group-one-lambda"])
def test_smallest_screen_sets_same_bits(hip, screen, n_lmda):
    d = _problem("lasso", np.float64, True, 1.0, screen=screen, n_lmda=n_lmda)
    st = _cold(d)
    on, off = _solve(st, True), _solve(st, False)
    assert on.error == "" and len(on.lmdas) == n_lmda
    _same_bits(on, off)
    assert on.counters["n_pin_launches"] == 1 and off.counters["n_pin_launches"] == n_lmda


@pytest.mark.parametrize("kind,dtype", [("lasso", np.float64), ("group", np.float64), ("lasso", np.float32)])
def test_continuation_from_a_solved_state(hip, kind, dtype):
    d = _problem(kind, dtype, True, 1.0)
    X = ad.matrix.dense(d["X"])
    six = np.concatenate([d["lmda_path"][:5], [dtype(0.8) * d["lmda_path"][4]]]).astype(dtype)
    full = _solve(_cold(d, design=X, lmda_path=six), True)
    head = _solve(_cold(d, design=X, lmda_path=six[:5]), True)
    assert full.error == "" and head.error == "" and len(head.lmdas) == 5
    nxt = ad.state.gaussian_pin_naive(
        X=X, y_mean=d["y_mean"], y_var=d["y_var"], constraints=None, groups=d["groups"], alpha=d["alpha"], penalty=d["penalty"],
        weights=d["w"], screen_set=d["screen"], lmda_path=[dtype(0.8) * head.lmdas[-1]], rsq=head.rsq, resid=head.resid,
        screen_beta=head.screen_beta, screen_is_active=head.screen_is_active, active_set_size=head.active_set_size,
        active_set=head.active_set, intercept=True, tol=1e-12, adev_tol=2, ddev_tol=-1, **_newton(dtype))
    out = _solve(nxt, True)
    tol = _atol(dtype)
    assert out.error == "" and len(out.lmdas) == 1
    assert np.abs(out.betas.toarray()[0] - full.betas.toarray()[5]).max() <= tol
    assert abs(out.intercepts[0] - full.intercepts[5]) <= tol
    assert abs(out.rsqs[0] - full.rsqs[5]) <= tol * d["y_var"]
    assert out.check(method="assert")


@pytest.mark.parametrize("kind", ["lasso", "group"])
def test_exit_rules_stop_both_routes_at_the_same_row(hip, kind):
    d, _, full, _ = _case(kind, np.float64, True, 1.0)
    r = full.rsqs.astype(np.float64)
    adev = 0.5 * (r[2] + r[3]) / d["y_var"]
    for launch in (True, False):
        out = _solve(_cold(d, adev_tol=adev), launch)
        assert out.error == "" and len(out.lmdas) == 4
        _same_bits(out, full, rows=4)
    inc = np.diff(r)                              # inc[l - 1] = rsqs[l] - rsqs[l - 1]
    thr = 0.5 * (inc[1] + inc[2])                 # halfway between two consecutive increments: fires at row 2 or 3 at the latest
    rows = next(l for l in range(1, L) if inc[l - 1] <= thr) + 1
    assert rows <= 4
    for launch in (True, False):
        out = _solve(_cold(d, ddev_tol=thr / d["y_var"]), launch)
        assert out.error == "" and len(out.lmdas) == rows
        _same_bits(out, full, rows=rows)


def test_max_iters_ends_the_path_with_the_reference_error(hip, caplog):
    d, _, full, _ = _case("lasso", np.float64, True, 1.0)
    outs = []
    with caplog.at_level(logging.ERROR, logger="adelie_amd"):
        for launch in (True, False):
            outs.append(_solve(_cold(d, max_iters=3), launch))
    on, off = outs
    assert "max coordinate descents reached at lambda index" in on.error and on.error == off.error
    k = len(on.lmdas)
    assert k < L and on.error.rstrip(".").endswith(str(k))
    assert any("max coordinate descents" in rec.getMessage() for rec in caplog.records)
    _same_bits(on, full, rows=k)
    _same_bits(on, off)


def test_max_active_size_ends_the_path_and_keeps_the_rows_before(hip):
    # the first float64 case in which at least 3 groups become active along the path
    d, _, full, _ = next(c for c in (_case(*k) for k in CASES if k[1] == np.float64) if c[2].active_set_size >= 3)
    on, off = (_solve(_cold(d, max_active_size=2), launch) for launch in (True, False))
    assert "Maximum number of active groups reached." in on.error and on.error == off.error
    k = len(on.lmdas)
    assert k < L and on.active_set_size <= 2
    _same_bits(on, full, rows=k)
    _same_bits(on, off)


# ---- covariance method ------------------------------------------------------------------------------------------------------
def _cov_state(d, A, lmda_path=None, **kw):
    nv = int(np.sum(d["sizes"][d["screen"]]))
    v = d["Xc"].T @ (d["w"].astype(np.float64) * d["yc"])
    args = dict(A=A, constraints=None, groups=d["groups"], alpha=d["alpha"], penalty=d["penalty"], screen_set=d["screen"],
                lmda_path=d["lmda_path"] if lmda_path is None else lmda_path, rsq=0.0, screen_beta=np.zeros(nv),
                screen_grad=v[d["cols"]], screen_is_active=np.zeros(len(d["screen"]), dtype=bool), active_set_size=0,
                active_set=np.zeros(len(d["screen"]), dtype=int), tol=1e-12, rdev_tol=-1, **_newton(d["dtype"]))
    args.update(kw)
    return ad.state.gaussian_pin_cov(**args), v


def _cov_designs(d):
    dtype = d["dtype"]
    w = d["w"].astype(np.float64)
    Amat = np.asfortranarray((d["Xc"].T @ (w[:, None] * d["Xc"])).astype(dtype))
    return {
        "dense": lambda: ad.matrix.dense(Amat, method="cov"),
        "lazy": lambda: ad.matrix.lazy_cov(np.asfortranarray((np.sqrt(w)[:, None] * d["Xc"]).astype(dtype))),
        "csc": lambda: ad.matrix.sparse(csc_matrix(Amat), method="cov", resident="csc"),
    }, Amat


@pytest.mark.parametrize("storage", ["dense", "lazy", "csc"])
@pytest.mark.parametrize("kind,dtype", [("lasso", np.float64), ("group", np.float64), ("lasso", np.float32)])
def test_pin_cov_agrees_with_pin_naive_and_between_routes(hip, storage, kind, dtype):
    d, _, naive, _ = _case(kind, dtype, False, 1.0)
    designs, Amat = _cov_designs(d)
    st, v = _cov_state(d, designs[storage]())
    on, off = _solve(st, True), _solve(st, False)
    tol = _atol(dtype)
    assert on.error == "" and len(on.lmdas) == L and not on.intercepts.any()
    assert np.abs(on.betas.toarray() - naive.betas.toarray()).max() <= tol
    assert np.abs(on.rsqs - naive.rsqs).max() <= tol * d["y_var"]
    beta = on.betas[-1].toarray().ravel().astype(np.float64)
    want = (v - Amat.astype(np.float64) @ beta)[d["cols"]]
    assert np.abs(on.screen_grad - want).max() <= (1e-12 if dtype == np.float64 else 1e-4)
    _same_bits(on, off, cov=True)
    _same_bits(on, _solve(st, True), cov=True)
    assert on.counters["n_pin_launches"] == 1 and off.counters["n_pin_launches"] == L
    assert on.check(method="assert")


def test_pin_cov_continuation_and_rdev_exit(hip):
    d, _, _, _ = _case("lasso", np.float64, False, 1.0)
    designs, _ = _cov_designs(d)
    A = designs["dense"]()
    six = np.concatenate([d["lmda_path"][:5], [0.8 * d["lmda_path"][4]]])
    full = _solve(_cov_state(d, A, lmda_path=six)[0], True)
    head = _solve(_cov_state(d, A, lmda_path=six[:5])[0], True)
    nxt, _ = _cov_state(d, A, lmda_path=[0.8 * head.lmdas[-1]], rsq=head.rsq, screen_beta=head.screen_beta,
                        screen_grad=head.screen_grad, screen_is_active=head.screen_is_active,
                        active_set_size=head.active_set_size, active_set=head.active_set)
    out = _solve(nxt, True)
    assert out.error == "" and len(out.lmdas) == 1
    assert np.abs(out.betas.toarray()[0] - full.betas.toarray()[5]).max() <= 1e-6
    assert abs(out.rsqs[0] - full.rsqs[5]) <= 1e-6 * d["y_var"]
    full = _solve(_cov_state(d, A)[0], True)
    r = full.rsqs.astype(np.float64)
    rel = np.diff(r) / r[1:]                       # rel[l - 1] = (rsqs[l] - rsqs[l - 1]) / rsqs[l]
    rdev = 0.5 * (rel[1] + rel[2])
    rows = next(l for l in range(1, L) if rel[l - 1] <= rdev) + 1
    assert rows <= 4
    for launch in (True, False):
        cut = _solve(_cov_state(d, A, rdev_tol=rdev)[0], launch)
        assert cut.error == "" and len(cut.lmdas) == rows
        _same_bits(cut, full, rows=rows)


# ---- the other designs and the per-lambda engines -----------------------------------------------------------------------------
def _calls_problem():
    d = _problem("lasso", np.float64, True, 1.0, seed=3)
    rng = np.random.default_rng(7)
    calls = rng.integers(0, 3, size=(N, P)).astype(np.int8)
    calls[rng.uniform(size=(N, P)) < 0.03] = -1
    snp = ad.matrix.snp_calldata(calls)
    Xd = calls.astype(np.float64)            # the numbers the design holds: missing calls imputed with the column mean
    for j in range(P):
        miss = calls[:, j] < 0
        Xd[miss, j] = calls[~miss, j].mean()
    return d, snp, np.asfortranarray(Xd)


def _repoint(d, Xd):
    """The problem of `d` on another matrix (same groups, screen set, weights; its own centring, path and cold start)."""
    e = dict(d)
    w = d["w"].astype(np.float64)
    rng = np.random.default_rng(11)
    beta = np.zeros(P)
    beta[d["cols"]] = rng.normal(size=len(d["cols"]))
    e["X"] = np.asfortranarray(Xd)
    e["y"] = Xd @ beta + 0.5 * rng.normal(size=N)
    e["y_mean"] = float(np.sum(w * e["y"]))
    e["yc"] = e["y"] - e["y_mean"]
    e["y_var"] = float(np.sum(w * e["yc"] ** 2))
    e["Xc"] = Xd - w @ Xd
    g0 = e["Xc"].T @ (w * e["yc"])
    lmax = max(abs(g0[g]) / d["penalty"][g] for g in d["screen"])
    e["lmda_path"] = 0.8 * lmax * 0.7 ** np.arange(L)
    return e


def test_snp_and_sparse_designs_agree_with_the_dense_design(hip):
    d, snp, Xd = _calls_problem()
    e = _repoint(d, Xd)
    dense = _solve(_cold(e), True)
    for design in (snp, ad.matrix.sparse(csc_matrix(Xd), resident="csc")):
        out = _solve(_cold(e, design=design), True)
        assert out.error == "" and len(out.lmdas) == L
        assert np.abs(out.betas.toarray() - dense.betas.toarray()).max() <= 1e-6
        assert np.abs(out.intercepts - dense.intercepts).max() <= 1e-6
        assert np.abs(out.rsqs - dense.rsqs).max() <= 1e-6 * e["y_var"]
        assert np.abs(out.resid - dense.resid).max() <= 1e-6


@pytest.mark.parametrize("ns,storage,route", [(160, "csc", 3), (300, "dense", 4)], ids=["block-engine", "panel-engine"])
def test_large_screen_sets_run_the_per_lambda_engines(hip, ns, storage, route):
    from oracle import oracle as orc

    orc.build()
    n, p = 400, 200 if ns <= 200 else 320
    screen = np.random.default_rng(5).permutation(p)[:ns]
    d = _problem("lasso", np.float64, True, 1.0, seed=2, n=n, p=p, screen=screen, n_lmda=4, unit_var=True)
    # (a design kept sparse has no panel engine under fixed weights: its fits run the block engine on the full Gram matrix)
    design = ad.matrix.dense(d["X"]) if storage == "dense" else ad.matrix.sparse(csc_matrix(d["X"]), resident="csc")
    out = _solve(_cold(d, design=design), True)
    assert out.error == "" and len(out.lmdas) == 4
    assert out.counters["pin_route"] == route
    assert (out.counters["n_panel_blocks"] > 0) == (route == 4)
    order = np.sort(screen)
    ref = ad.grpnet(orc.dense(np.asfortranarray(d["X"][:, order])), ad.glm.gaussian(d["y"], weights=d["w"]),
                    penalty=d["penalty"][order], intercept=True, lmda_path=d["lmda_path"], early_exit=False, tol=1e-12,
                    progress_bar=False)
    B = np.zeros((4, p))
    B[:, order] = ref.betas.toarray()
    assert np.abs(out.betas.toarray() - B).max() <= 1e-6
    assert np.abs(out.intercepts - ref.intercepts).max() <= 1e-6
    assert np.abs(out.rsqs - np.asarray(ref.devs) * d["y_var"]).max() <= 1e-6 * d["y_var"]
    assert out.check(method="assert")
