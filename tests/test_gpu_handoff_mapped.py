"""A Gaussian lambda's hand-off through host-mapped memory (Solver::fit_handoff in solver_fit.hpp, the scores of
device_abs_grad) against the copy route of ADELIE_HIP_HANDOFF=copies: every case solves twice in one process and asserts byte equality of lmdas,
intercepts, devs, betas, the final grad and the counters."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import adelie_amd as ad

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def same(a, b):
    assert a.error == "" and b.error == "", (a.error, b.error)
    assert bits(a.lmdas) == bits(b.lmdas) and bits(a.intercepts) == bits(b.intercepts) and bits(a.devs) == bits(b.devs)
    A, B = a.betas.tocsr(), b.betas.tocsr()
    assert bits(A.indptr) == bits(B.indptr) and bits(A.indices) == bits(B.indices) and bits(A.data) == bits(B.data)
    assert bits(a.grad) == bits(b.grad) and bits(a.abs_grad) == bits(b.abs_grad)
    assert a.counters == b.counters, {k: (a.counters[k], b.counters[k]) for k in a.counters if a.counters[k] != b.counters[k]}


def both(monkeypatch, solve):
    """`solve()` on the default route, then through copies."""
    monkeypatch.delenv("ADELIE_HIP_HANDOFF", raising=False)
    mapped = solve()
    monkeypatch.setenv("ADELIE_HIP_HANDOFF", "copies")
    copies = solve()
    monkeypatch.delenv("ADELIE_HIP_HANDOFF", raising=False)
    same(mapped, copies)
    return mapped


def data(n, p, nnz, seed, dtype=np.float64):
    rng = np.random.RandomState(seed)
    X = np.asfortranarray(rng.normal(size=(n, p)).astype(dtype))
    beta = np.zeros(p)
    beta[rng.choice(p, min(nnz, p), replace=False)] = rng.normal(size=min(nnz, p)) * 2
    y = (X.astype(np.float64) @ beta + rng.normal(size=n)).astype(dtype)
    return X, y


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("G,gs", [(1, 1), (63, 1), (64, 1), (65, 1), (1025, 1), (205, 5)])
def test_group_count_tails_of_the_score_kernel(hip, monkeypatch, G, gs, dtype):
    """n = 130 is no multiple of the wave or of 16 bytes / 8; G = 1025 is one past four workgroups of the score kernel."""
    X, y = data(130, G * gs, 8, seed=G + gs, dtype=dtype)
    # (float32 with n < p: a path down to 0.1 lambda_max at a tolerance single precision reaches)
    kw = dict(lmda_path_size=12, early_exit=False, min_ratio=0.1, tol=1e-4 if dtype == np.float32 else 1e-10)
    if gs > 1:
        kw.update(groups=np.arange(0, G * gs, gs), alpha=0.5)
        if dtype == np.float32:  # (the default newton_tol = 1e-12 is below float32 resolution: the root find then reports max iterations)
            kw.update(newton_tol=1e-5)
    both(monkeypatch, lambda: ad.grpnet(ad.matrix.dense(X), ad.glm.gaussian(y), **kw))


@pytest.fixture(scope="module")
def crossing():
    return data(600, 400, 200, seed=5)


@pytest.mark.parametrize("intercept", [True, False])
def test_path_from_the_single_workgroup_kernel_into_the_panel_engine(hip, monkeypatch, crossing, intercept):
    """The screen set passes 128 values in the path: the fits before it run cd_lasso_kernel (their scalars travel through
    d_sc), those after it the panel engine with speculative passes, whose hand-off is the fused launch.  Without an intercept
    the mean vector is absent from the argument records."""
    X, y = crossing
    kw = dict(lmda_path_size=30, early_exit=False, tol=1e-10, intercept=intercept)
    s = both(monkeypatch, lambda: ad.grpnet(ad.matrix.dense(X), ad.glm.gaussian(y), **kw))
    assert s.counters["n_speculated"] > 0 and s.counters["n_panel_blocks"] > 0
    assert len(s.screen_set) > 128


@pytest.mark.parametrize("panel", [False, True])
@pytest.mark.parametrize("unpenalised", [False, True])
def test_path_with_filtered_sweeps(hip, monkeypatch, unpenalised, panel):
    """The path case of test_gpu_filter_fused.py.  Its screen set stays under 20 values, so as it stands every fit is the
    single-workgroup kernel's and the four words of a filtered sweep come by their download on both routes.  With the panel
    engine taken from the first screen value on, the sweep goes out behind a panel fit and a speculative pass follows: the four
    words travel in fit_handoff's launch, or by the download when no pass follows."""
    rng = np.random.RandomState(39)
    n, p = 9000, 200
    X = np.asfortranarray(rng.normal(size=(n, p)))
    beta = np.zeros(p)
    beta[rng.choice(p, 10, replace=False)] = rng.normal(size=10) * 2
    y = X @ beta + rng.normal(size=n)
    pen = np.ones(p)
    if unpenalised:
        pen[7] = 0.0
    monkeypatch.setenv("ADELIE_HIP_FILTER_SWEEP", "1")
    if panel:
        monkeypatch.setenv("ADELIE_HIP_CD_BLOCK_MIN_NV", "1")
    kw = dict(lmda_path_size=30, early_exit=False, tol=1e-9, penalty=pen)
    s = both(monkeypatch, lambda: ad.grpnet(ad.matrix.dense(X), ad.glm.gaussian(y), **kw))
    assert s.counters["n_sweeps_filtered"] > 0
    if panel:
        assert s.counters["n_panel_blocks"] > 0 and s.counters["n_speculated"] > 0
    else:
        assert s.counters["n_panel_blocks"] == 0


def test_open_list_beyond_its_cap_is_refilled_behind_a_panel_fit(hip, monkeypatch, capfd):
    """Under the rule of ADELIE_HIP_FILTER_DEPTH=0 the threshold lies at the score twice as deep as screen() may read, about
    3.2 |S| groups outside the screen set; the list holds max(1024, p / 4) = 1024 columns at p = 4000.  Once the screen set
    passes some 330 groups (the panel engine has long taken over: its fits hand over in the fused launch) a filtered sweep
    overflows: the flag comes back among the four words, and ensure_exact_grad sweeps the snapshot of the residual that
    launch took.  The trace line of each filtered sweep carries the flags word: bit 0 is the overflow."""
    X, y = data(1000, 4000, 250, seed=1)
    monkeypatch.setenv("ADELIE_HIP_FILTER_SWEEP", "1")
    monkeypatch.setenv("ADELIE_HIP_FILTER_DEPTH", "0")
    monkeypatch.setenv("ADELIE_HIP_TRACE", "1")
    traces = []

    def solve():
        capfd.readouterr()
        st = ad.grpnet(ad.matrix.dense(X), ad.glm.gaussian(y), lmda_path_size=30, early_exit=False, tol=1e-9)
        traces.append(capfd.readouterr().err)
        return st

    s = both(monkeypatch, solve)
    assert s.counters["n_sweeps_filtered"] > 0 and s.counters["n_sweeps_refilled"] > 0
    assert s.counters["n_panel_blocks"] > 0 and s.counters["n_speculated"] > 0
    for trace in traces:
        flags = [int(line.split(" flags ")[1].split()[0]) for line in trace.splitlines() if line.startswith("[fsweep]")]
        assert any(f & 1 for f in flags), flags


def test_a_speculative_pass_taken_back(hip, monkeypatch, crossing):
    """A live read of the residual in the middle of the path takes the speculative pass back: the snapshots it is rolled back
    to are the ones the fused launch took."""
    X, y = crossing
    seen = {}

    def solve():
        got = []

        def peek(s):
            if s.n_solutions in (22, 27):
                got.append(np.array(s.resid, copy=True))
            return False

        st = ad.grpnet(ad.matrix.dense(X), ad.glm.gaussian(y), progress_bar=False, exit_cond=peek, early_exit=False,
                       lmda_path_size=30, tol=1e-10)
        seen[len(seen)] = got
        return st

    s = both(monkeypatch, solve)
    assert s.counters["n_spec_rollbacks"] > 0
    assert [bits(r) for r in seen[0]] == [bits(r) for r in seen[1]] and len(seen[0]) == 2


def test_two_solves_in_flight_on_alias_handles(hip, monkeypatch, crossing):
    """The mapped block is per solver: two paths in flight on two threads equal the path solved alone."""
    X, y = crossing
    monkeypatch.delenv("ADELIE_HIP_HANDOFF", raising=False)
    kw = dict(lmda_path_size=30, early_exit=False, tol=1e-10)
    Xd = ad.matrix.dense(X)
    alone = ad.grpnet(Xd, ad.glm.gaussian(y), **kw)
    y2 = y[::-1].copy()
    alone2 = ad.grpnet(Xd, ad.glm.gaussian(y2), **kw)
    handles = [Xd, Xd.alias()]
    with ThreadPoolExecutor(max_workers=2) as pool:
        a, b = pool.map(lambda hy: ad.grpnet(hy[0], ad.glm.gaussian(hy[1]), **kw), zip(handles, (y, y2)))
    same(a, alone)
    same(b, alone2)
