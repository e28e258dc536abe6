"""The filtered invariance sweep through the 16-bit shadow copy (ADELIE_HIP_SHADOW_KIND=q15: int16 values, one f64 scale per
column) and the rule that picks a design's kind (auto).  Kernel level through adelie_hip_filter_sweep_test and the helpers of
test_gpu_filter_sweep / test_gpu_filter_fused; every case asserts what check_filtered asserts -- exact columns carry the full
sweep's bytes, unlisted columns lie within the bound, whole groups only, two runs bit-identical -- with the bound restated in
numpy from the encoding (test_shadow_kind_host.q15_bounds)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import adelie_amd as ad
import test_gpu_filter_sweep as base
from test_gpu_filter_fused import clean, scores
from test_gpu_filter_sweep import bounds as f32_bounds
from test_gpu_filter_sweep import assert_identical, check_filtered, fsweep, group_norms, make_data, make_problem
from test_shadow_kind_host import q15_bounds, q15_err_nrm

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture
def q15(monkeypatch):
    """Every copy made in the test is q15, and check_filtered measures against the q15 bound."""
    monkeypatch.setenv("ADELIE_HIP_SHADOW_KIND", "q15")
    monkeypatch.setattr(base, "bounds", q15_bounds)
    return monkeypatch


@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    """(splits of the f64 sweep, of the float32 shadow, of the q15 shadow, the q15 panel width, its ld padding) from
    adelie_amd/csrc/sweep_shape.hpp itself, compiled for the host."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is required (the oracle needs one as well)"
    exe = str(tmp_path_factory.mktemp("q15_shape") / "q15_shape")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-o", exe, os.path.join(HERE, "native", "shadow_q15_shape_main.cpp")])

    def counts(n, p):
        return tuple(int(t) for t in subprocess.check_output([exe, str(n), str(p)], text=True).split())

    return counts


def is_q15(Xd, X=None):
    info = Xd.shadow_info()
    assert info["kind"] == "q15", info
    if X is not None:
        n, p = X.shape
        assert info["bytes"] == p * (-(-n // 64) * 64) * 2 + 3 * p * 8
    return info


# ---- forced q15, kernel level ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,p,gs,intercept", [(5000, 37, 1, True), (5000, 37, 4, False), (1000, 4100, 1, True)])
def test_q15_against_full_sweep(hip, q15, n, p, gs, intercept):
    prob = make_problem(n, p, gs, seed=n + p + gs, intercept=intercept)
    X, w, r, rsum, xm, groups, gsizes, pen = prob
    Xd = ad.matrix.dense(X)
    screen = list(range(0, len(groups), 7))
    score = group_norms(X.T @ (w * r) - rsum * (xm if xm is not None else 0), groups, gsizes) / pen
    _, _, mask, info = check_filtered(q15, Xd, X, prob, screen, np.quantile(score, 0.9))
    assert info[1] == 0 and 0 < info[0] < p and not mask.all()
    scols = sum(int(gsizes[g]) for g in screen)
    _, _, maski, infoi = check_filtered(q15, Xd, X, prob, screen, np.inf)
    assert infoi[0] == 0 and maski.sum() == scols
    assert Xd.shadow_stats() == {"state": 1, "builds": 1, "ineligible": 0}
    info = is_q15(Xd, X)
    assert 1e-5 < info["err_median"] <= info["err_max"] < 1e-4   # Gaussian columns: about 4e-5 of their norm


@pytest.mark.parametrize("n", [5001, 5002, 5003, 5004, 5005, 5006, 5007])
def test_q15_row_counts_ending_inside_a_load(hip, q15, n):
    prob = make_problem(n, 19, 1, seed=n)
    Xd = ad.matrix.dense(prob[0])
    _, _, mask, info = clean(q15, Xd, prob, [3, 18], np.quantile(scores(prob), 0.8))
    assert 0 < info[0] and not mask.all()
    is_q15(Xd, prob[0])


def test_q15_odd_leading_dimension_and_single_row(hip, q15):
    import torch

    prob = make_problem(1001, 60, 1, seed=5)
    Xt = torch.from_numpy(np.ascontiguousarray(prob[0].T)).cuda().T
    Xd = ad.matrix.dense(Xt)
    _, _, mask, info = clean(q15, Xd, prob, [0, 11, 59], np.quantile(scores(prob), 0.8))
    assert 0 < info[0] and not mask.all()
    is_q15(Xd, prob[0])
    prob = make_problem(1, 9, 1, seed=6, zero_w=False)   # n = 1: every q is +-32767
    Xd = ad.matrix.dense(prob[0])
    check_filtered(q15, Xd, prob[0], prob, [], np.inf)
    check_filtered(q15, Xd, prob[0], prob, [], 0.0)
    is_q15(Xd, prob[0])


@pytest.mark.parametrize("which", ["one", "cb-1", "cb", "cb+1", "2cb+1"])
def test_q15_panel_tails(hip, q15, shapes, which):
    cb = shapes(600, 8)[3]
    assert cb in (8, 16)
    p = {"one": 1, "cb-1": cb - 1, "cb": cb, "cb+1": cb + 1, "2cb+1": 2 * cb + 1}[which]
    prob = make_problem(600, p, 1, seed=36 + p)
    Xd = ad.matrix.dense(prob[0])
    _, _, mask, _ = clean(q15, Xd, prob, [p - 1] if p > 1 else [], np.quantile(scores(prob), 0.7))
    clean(q15, Xd, prob, [], np.inf)
    assert mask.sum() >= 1
    is_q15(Xd, prob[0])


@pytest.mark.parametrize("n,p", [(9000, 40), (20000, 24)])
def test_q15_row_splits_of_the_two_bodies_differ(hip, q15, shapes, n, p):
    """The exact part of the launch takes the full f64 sweep's row splits, the q15 part its own: 2048 rows per workgroup and
    iteration, where the float32 kind has 1024.  At both shapes the three counts differ from one another."""
    ns_f64, ns_f32, ns_q15, _, _ = shapes(n, p)
    assert ns_q15 > 1 and len({ns_f64, ns_f32, ns_q15}) == 3, (ns_f64, ns_f32, ns_q15)
    prob = make_problem(n, p, 1, seed=31 + p)
    Xd = ad.matrix.dense(prob[0])
    _, _, mask, info = clean(q15, Xd, prob, [2, 17, p - 1], np.quantile(scores(prob), 0.8))
    assert 0 < info[0] < p - 3 and not mask.all()
    is_q15(Xd, prob[0])


def test_q15_zero_binary_tiny_and_extreme_columns(hip, q15):
    rng = np.random.RandomState(9)
    prob = list(make_problem(2000, 40, 1, seed=9))
    X = prob[0]
    X[:, 2] = 0.0                                     # zero column: scale 0, all q 0
    X[:, 3] *= 1e-300                                 # tiny: the scale is 1e-300 / 32767, still a normal number
    X[:, 5] = (rng.uniform(size=2000) < 0.4)          # 0/1: the copy is the column itself
    X[:, 7] = np.where(rng.uniform(size=2000) < 0.5, -4.0, 4.0)   # every entry at +-max
    X[:, 9] *= 1e150                                  # far beyond FLT_MAX
    X[0, 11], X[1, 11] = np.abs(X[:, 11]).max() * 4, -np.abs(X[:, 11]).max() * 4   # the extremes are +-32767 exactly
    prob[4] = X.T @ prob[1]
    e, nx = q15_err_nrm(X)
    assert e[2] == 0 and nx[2] == 0 and e[5] == 0 and e[7] == 0 and 0 < e[3] < 1e-300 and e[9] > 1e140
    Xd = ad.matrix.dense(X)
    with np.errstate(over="ignore"):
        full, got, mask, info = check_filtered(q15, Xd, X, prob, [1], np.inf)
        assert info[1] == 0 and not mask[[2, 3, 5, 7, 11]].any()
        # a column whose copy is the column itself: the two sweeps differ by rounding alone
        for j in (5, 7):
            assert abs(got[j] - full[j]) <= (4 * 2000 + 8) * 2.0 ** -53 * nx[j] * np.sqrt(((prob[1] * prob[2]) ** 2).sum()) * (1 + 1e-6)
        assert got[2] == 0.0
        check_filtered(q15, Xd, X, prob, [1], np.quantile(scores(prob), 0.8))
    is_q15(Xd, X)
    # all columns 0/1: the largest e_j the library measured is 0
    B = np.asfortranarray((rng.uniform(size=(500, 12)) < 0.3).astype(np.float64))
    probB = list(make_problem(500, 12, 1, seed=10))
    probB[0] = B
    probB[4] = B.T @ probB[1]
    Bd = ad.matrix.dense(B)
    check_filtered(q15, Bd, B, probB, [0], np.inf)
    assert is_q15(Bd, B)["err_max"] == 0.0


def test_q15_open_list_of_length_zero_one_and_beyond_the_cap(hip, q15):
    p = 4100
    prob = make_problem(1000, p, 1, seed=37)
    Xd = ad.matrix.dense(prob[0])
    screen = [5, 4000]
    s = scores(prob)
    s[screen] = -1
    top = np.sort(s)[-2:]
    _, _, mask, info = clean(q15, Xd, prob, screen, np.inf)
    assert info[0] == 0 and mask.sum() == 2
    # between the two largest scores outside the screen set, which lie many q15 bounds apart
    bnd = q15_bounds(prob[0], prob[1] * prob[2]) / prob[7]
    assert top[1] - top[0] > 20 * bnd.max()
    _, _, mask, info = clean(q15, Xd, prob, screen, 0.5 * (top[0] + top[1]))
    assert info[0] == 1 and mask[int(np.argmax(s))] and mask.sum() == 3
    with np.errstate(divide="ignore", invalid="ignore"):
        _, _, mask, info = check_filtered(q15, Xd, prob[0], prob, screen, 0.0)
    cap = max(1024, p // 4)
    assert info[1] == 1 and info[0] == cap and info[3] == p - 2 and mask.sum() == cap + 2
    is_q15(Xd, prob[0])


def test_q15_modified_screen_column_raises_the_flag(hip, q15):
    import torch

    prob = make_problem(2000, 40, 1, seed=38)
    X, w, r, rsum, xm, groups, gsizes, pen = prob
    Xt = torch.from_numpy(np.ascontiguousarray(X.T)).cuda().T
    Xd = ad.matrix.dense(Xt)
    q15.setenv("ADELIE_HIP_FILTER_SWEEP", "1")
    _, _, info = fsweep(Xd, w, r, rsum, xm, [4, 20], groups, gsizes, pen, np.inf)
    assert info[2] == 1 and info[1] == 0 and Xd.shadow_stats()["state"] == 1
    is_q15(Xd, X)
    Xt[:, 20] *= 1.5
    torch.cuda.synchronize()
    got, mask, info = fsweep(Xd, w, r, rsum, xm, [4, 20], groups, gsizes, pen, np.inf)
    assert info[2] == 1 and info[1] & 2
    assert Xd.shadow_stats()["state"] == -1 and Xd.shadow_info()["kind"] is None   # retired
    full, _, info_full = fsweep(Xd, w, r, rsum, xm, [4, 20], groups, gsizes, pen, np.inf)
    assert info_full[2] == 0 and got[mask].tobytes() == full[mask].tobytes() and mask.sum() == 2


def test_q15_design_with_an_entry_that_is_not_finite(hip, q15):
    prob = list(make_problem(2000, 40, 1, seed=9))
    X = prob[0]
    X[0, 5] = np.inf
    Xd = ad.matrix.dense(X)
    q15.setenv("ADELIE_HIP_FILTER_SWEEP", "1")
    X, w, r, rsum, xm, groups, gsizes, pen = prob
    _, mask, info = fsweep(Xd, w, r, rsum, None, [1], groups, gsizes, pen, np.inf)
    assert info[2] == 0 and mask.all()
    st = Xd.shadow_stats()
    assert st["state"] == -1 and st["ineligible"] == 1 and Xd.shadow_info()["kind"] is None


# ---- auto --------------------------------------------------------------------------------------------------------------------
def one_sweep(monkeypatch, X, seed=3):
    prob = list(make_problem(X.shape[0], X.shape[1], 1, seed=seed))
    prob[0] = X
    prob[4] = X.T @ prob[1]
    Xd = ad.matrix.dense(X)
    check_filtered(monkeypatch, Xd, X, prob, [1], np.quantile(scores(prob), 0.8))
    return Xd


def test_auto_gives_a_gaussian_design_q15(hip, monkeypatch):
    X = np.asfortranarray(np.random.RandomState(0).normal(size=(2000, 24)))
    f32_bytes = 2000 * 24 * 4
    for kind_word, min_bytes, expect in ((None, 1, "q15"), ("auto", 1, "q15"), (None, f32_bytes, "q15"), (None, f32_bytes + 1, "f32")):
        if kind_word is None:
            monkeypatch.delenv("ADELIE_HIP_SHADOW_KIND", raising=False)
        else:
            monkeypatch.setenv("ADELIE_HIP_SHADOW_KIND", kind_word)
        monkeypatch.setenv("ADELIE_HIP_SHADOW_MIN_BYTES", str(min_bytes))
        monkeypatch.setattr(base, "bounds", q15_bounds if expect == "q15" else f32_bounds)
        Xd = one_sweep(monkeypatch, X)
        assert Xd.shadow_info()["kind"] == expect
        assert Xd.shadow_stats() == {"state": 1, "builds": 1, "ineligible": 0}


def test_auto_gives_a_design_with_outliers_float32(hip, monkeypatch):
    """20000 x 16, one entry of 200 standard deviations in 4 of the 16 columns (more than 1/8): e_j / ||x_j|| of those
    columns is 2 * 2^-11, of the others 4e-5.  With outliers in 2 columns (1/8) the design still gets q15."""
    rng = np.random.RandomState(1)
    X = np.asfortranarray(rng.normal(size=(20000, 16)))
    out = [1, 6, 10, 15]
    for j in out:
        X[100 + j, j] = 200.0
    e, nx = q15_err_nrm(X)
    ratio = e / np.sqrt((X ** 2).sum(axis=0))
    rest = np.setdiff1d(np.arange(16), out)
    assert (ratio[out] > 2 * 2.0 ** -11).all() and (ratio[out] < 2.3 * 2.0 ** -11).all() and (ratio[rest] < 2.0 ** -11 / 8).all()
    monkeypatch.setenv("ADELIE_HIP_SHADOW_MIN_BYTES", "1")
    Xd = one_sweep(monkeypatch, X)          # (check_filtered with the float32 bound)
    info = Xd.shadow_info()
    assert info["kind"] == "f32" and info["bytes"] == 16 * 20000 * 4 + 2 * 16 * 8 and info["err_max"] < 1e-7
    assert Xd.shadow_stats() == {"state": 1, "builds": 2, "ineligible": 0}   # the q15 copy was made, measured and dropped
    X2 = X.copy(order="F")
    X2[100 + 6, 6] = 1.0
    X2[100 + 15, 15] = 1.0
    monkeypatch.setattr(base, "bounds", q15_bounds)
    info = is_q15(one_sweep(monkeypatch, X2), X2)
    assert 2 * 2.0 ** -11 < info["err_max"] < 2.3 * 2.0 ** -11 and info["err_median"] < 1e-4


# every shape the tests above sweep (the panel tails at either width the kernel may be built with)
SHAPES_ABOVE = ([(5000, 37), (1000, 4100), (1001, 60), (1, 9), (9000, 40), (20000, 24), (2000, 40), (500, 12), (2000, 24), (20000, 16),
                 (300, 2000)] + [(n, 19) for n in range(5001, 5008)] + [(600, p) for p in (1, 7, 8, 9, 15, 16, 17, 33)])


@pytest.mark.parametrize("n,p", SHAPES_ABOVE)
def test_auto_with_the_default_threshold_stays_float32(hip, monkeypatch, n, p):
    monkeypatch.delenv("ADELIE_HIP_SHADOW_MIN_BYTES", raising=False)
    monkeypatch.delenv("ADELIE_HIP_SHADOW_KIND", raising=False)
    prob = make_problem(n, p, 1, seed=n + p, zero_w=n > 1)
    Xd = ad.matrix.dense(prob[0])
    check_filtered(monkeypatch, Xd, prob[0], prob, [0], np.inf)
    info = Xd.shadow_info()
    assert info["kind"] == "f32" and info["bytes"] == p * (-(-n // 4) * 4) * 4 + 2 * p * 8
    assert ad.matrix.dense(prob[0]).shadow_info() == {"kind": None, "bytes": 0, "err_median": 0.0, "err_max": 0.0}


# ---- solver level ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["lasso", "groups", "weights"])
def test_paths_are_bit_identical_off_float32_and_q15(hip, monkeypatch, variant):
    X, y = make_data()   # 300 x 2000
    kw = dict(lmda_path_size=30, early_exit=False, tol=1e-9)
    w = None
    if variant == "groups":
        kw.update(groups=np.arange(0, X.shape[1], 4), alpha=0.5)
    if variant == "weights":
        w = np.random.RandomState(3).uniform(0.5, 1.5, size=len(y))
        w[::4] = 0
        w /= w.sum()
    out = {}
    for arm, sweep, kind in (("off", "0", "f32"), ("f32", "1", "f32"), ("q15", "1", "q15")):
        monkeypatch.setenv("ADELIE_HIP_FILTER_SWEEP", sweep)
        monkeypatch.setenv("ADELIE_HIP_SHADOW_KIND", kind)
        Xd = ad.matrix.dense(X)
        out[arm] = ad.grpnet(Xd, ad.glm.gaussian(y, weights=w), **kw)
        assert Xd.shadow_info()["kind"] == (None if arm == "off" else kind)
    assert out["off"].counters["n_sweeps_filtered"] == 0
    for arm in ("f32", "q15"):
        assert_identical(out[arm], out["off"], state_too=True)
        print(variant, arm, {k: out[arm].counters[k] for k in base.NEW_COUNTERS}, "of", out[arm].counters["n_sweeps"], "sweeps")
        assert out[arm].counters["n_sweeps_filtered"] > 0
