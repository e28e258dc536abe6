"""The filtered invariance sweep whose beforehand-known exact columns (screen groups, groups without a penalty) run inside
the shadow launch and are reduced, guarded and stored by the classification step (adelie_hip_filter_sweep_test, the same
enqueue function the solver calls).  Every case asserts what test_gpu_filter_sweep.check_filtered asserts: exact columns
carry the full sweep's bytes, unlisted columns lie within `bounds`, whole groups only, two runs identical; and, unless
the case is about a flag, that the flags word is 0."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import adelie_amd as ad
from test_gpu_filter_sweep import assert_identical, check_filtered, fsweep, group_norms, make_problem, on_off

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def scores(prob):
    X, w, r, rsum, xm, groups, gsizes, pen = prob
    g = X.T @ (w * r) - (rsum * xm if xm is not None else 0.0)
    with np.errstate(divide="ignore"):
        return group_norms(g, groups, gsizes) / pen


def clean(monkeypatch, Xd, prob, screen, tstar):
    """check_filtered, the flags word 0, and the exact mask = screen columns + unpenalised columns + listed columns, none
    counted twice."""
    groups, gsizes, pen = prob[5], prob[6], prob[7]
    with np.errstate(divide="ignore", invalid="ignore"):
        full, got, mask, info = check_filtered(monkeypatch, Xd, prob[0], prob, screen, tstar)
    assert info[1] == 0
    before = set(screen) | {g for g in range(len(groups)) if not pen[g] > 0}
    assert mask.sum() == info[0] + sum(int(gsizes[g]) for g in before)
    return full, got, mask, info


@pytest.fixture(scope="module")
def split_counts(tmp_path_factory):
    """(f64 sweep with 16-byte loads, f64 sweep with scalar loads, shadow sweep, the shadow's panel width) from
    adelie_amd/csrc/sweep_shape.hpp itself, compiled for the host."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is required (the oracle needs one as well)"
    exe = str(tmp_path_factory.mktemp("sweep_shape") / "sweep_shape")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-o", exe, os.path.join(HERE, "native", "sweep_shape_main.cpp")])

    def counts(n, p):
        return tuple(int(t) for t in subprocess.check_output([exe, str(n), str(p)], text=True).split())

    return counts


def test_the_two_bodies_of_one_launch_split_the_rows_differently(hip, monkeypatch, split_counts):
    """n = 9000, p = 40: the exact part of the launch takes the full f64 sweep's row splits, the shadow part its own."""
    ns_f64, _, ns_shadow, _ = split_counts(9000, 40)
    assert ns_f64 != ns_shadow and ns_f64 > 1 and ns_shadow > 1, (ns_f64, ns_shadow)
    prob = make_problem(9000, 40, 1, seed=31)
    Xd = ad.matrix.dense(prob[0])
    _, _, mask, info = clean(monkeypatch, Xd, prob, [2, 17, 39], np.quantile(scores(prob), 0.8))
    assert 0 < info[0] < 37 and not mask.all()


def test_no_exact_part(hip, monkeypatch):
    prob = make_problem(600, 37, 1, seed=32)
    Xd = ad.matrix.dense(prob[0])
    _, _, mask, info = clean(monkeypatch, Xd, prob, [], np.quantile(scores(prob), 0.8))
    assert 0 < info[0] == mask.sum() < 37
    clean(monkeypatch, Xd, prob, [], np.inf)


@pytest.mark.parametrize("n,p", [(600, 9), (600, 37), (1, 9)])
def test_every_group_screened(hip, monkeypatch, n, p):
    prob = make_problem(n, p, 1, seed=33 + p, zero_w=n > 1)
    Xd = ad.matrix.dense(prob[0])
    for tstar in (np.inf, 0.0):
        _, _, mask, info = clean(monkeypatch, Xd, prob, list(range(p)), tstar)
        assert mask.all() and info[0] == 0 and info[3] == 0


def test_unpenalised_group_next_to_screen_groups(hip, monkeypatch):
    prob = list(make_problem(600, 37, 4, seed=34))   # ten groups, the last of one column
    prob[7] = prob[7].copy()
    prob[7][3] = 0.0
    Xd = ad.matrix.dense(prob[0])
    s = scores(prob)
    _, _, mask, info = clean(monkeypatch, Xd, prob, [1, 9], np.quantile(s[np.isfinite(s)], 0.6))
    assert mask[12:16].all() and mask[4:8].all() and mask[36] and 0 < info[0] and not mask.all()
    # the unpenalised group in the screen set as well (where a solver keeps it): swept in both lists, same bits
    with np.errstate(divide="ignore", invalid="ignore"):
        _, _, mask2, info2 = check_filtered(monkeypatch, Xd, prob[0], prob, [1, 3, 9], np.inf)
    assert info2[1] == 0 and info2[0] == 0 and mask2.sum() == 9


def test_unaligned_exact_part(hip, monkeypatch):
    """An adopted column-major tensor with n = 1001: the f64 body of the fused launch takes scalar loads, the shadow keeps
    its own padded leading dimension."""
    import torch

    prob = make_problem(1001, 60, 1, seed=35)
    Xt = torch.from_numpy(np.ascontiguousarray(prob[0].T)).cuda().T
    Xd = ad.matrix.dense(Xt)
    _, _, mask, info = clean(monkeypatch, Xd, prob, [0, 11, 59], np.quantile(scores(prob), 0.8))
    assert 0 < info[0] and not mask.all()


@pytest.mark.parametrize("p", [1, 7, 8, 9, 17])
def test_panel_tails_of_the_shadow(hip, monkeypatch, p, split_counts):
    cb = split_counts(600, p)[3]
    assert {q % cb for q in (1, 7, 8, 9, 17)} >= {0, 1, cb - 1}   # full, one-column and one-short tail panels at this width
    prob = make_problem(600, p, 1, seed=36 + p)
    Xd = ad.matrix.dense(prob[0])
    _, _, mask, _ = clean(monkeypatch, Xd, prob, [p - 1] if p > 1 else [], np.quantile(scores(prob), 0.7))
    clean(monkeypatch, Xd, prob, [], np.inf)
    assert mask.sum() >= 1


def test_open_list_of_length_zero_one_and_beyond_the_cap(hip, monkeypatch):
    p = 4100
    prob = make_problem(1000, p, 1, seed=37)
    Xd = ad.matrix.dense(prob[0])
    screen = [5, 4000]
    s = scores(prob)
    s[screen] = -1
    top = np.sort(s)[-2:]
    _, _, mask, info = clean(monkeypatch, Xd, prob, screen, np.inf)
    assert info[0] == 0 and mask.sum() == 2
    # below the largest non-screen score, above the second (half their distance is far beyond a float32 shadow's bound)
    _, _, mask, info = clean(monkeypatch, Xd, prob, screen, 0.5 * (top[0] + top[1]))
    assert info[0] == 1 and mask[int(np.argmax(s))] and mask.sum() == 3
    # everything wanted: the cap of max(1024, p / 4) = 1025 overflows, the flag says so (check_filtered compares two runs)
    with np.errstate(divide="ignore", invalid="ignore"):
        _, _, mask, info = check_filtered(monkeypatch, Xd, prob[0], prob, screen, 0.0)
    cap = max(1024, p // 4)
    assert info[1] == 1 and info[0] == cap and info[3] == p - 2 and mask.sum() == cap + 2


def test_a_modified_screen_column_raises_the_flag(hip, monkeypatch):
    """The guard of the screen columns runs in the classification step now: a screen column changed after the shadow was
    made leaves its bound there."""
    import torch

    prob = make_problem(2000, 40, 1, seed=38)
    X, w, r, rsum, xm, groups, gsizes, pen = prob
    Xt = torch.from_numpy(np.ascontiguousarray(X.T)).cuda().T
    Xd = ad.matrix.dense(Xt)
    monkeypatch.setenv("ADELIE_HIP_FILTER_SWEEP", "1")
    _, _, info = fsweep(Xd, w, r, rsum, xm, [4, 20], groups, gsizes, pen, np.inf)
    assert info[2] == 1 and info[1] == 0 and Xd.shadow_stats()["state"] == 1
    Xt[:, 20] *= 1.5
    torch.cuda.synchronize()
    X2 = X.copy(order="F")
    X2[:, 20] *= 1.5
    got, mask, info = fsweep(Xd, w, r, rsum, xm, [4, 20], groups, gsizes, pen, np.inf)
    assert info[2] == 1 and info[1] & 2
    assert Xd.shadow_stats()["state"] == -1   # retired: the next sweep of this design is the full one
    # the exact columns are still the full sweep of the design as it is now
    full, _, info_full = fsweep(Xd, w, r, rsum, xm, [4, 20], groups, gsizes, pen, np.inf)
    assert info_full[2] == 0 and got[mask].tobytes() == full[mask].tobytes() and mask.sum() == 2
    assert np.allclose(full, X2.T @ (w * r) - rsum * xm, rtol=1e-9, atol=1e-12)


def test_path_with_an_unpenalised_column_hook_on_and_off(hip, monkeypatch):
    rng = np.random.RandomState(39)
    n, p = 9000, 200
    X = np.asfortranarray(rng.normal(size=(n, p)))
    beta = np.zeros(p)
    beta[rng.choice(p, 10, replace=False)] = rng.normal(size=10) * 2
    y = X @ beta + rng.normal(size=n)
    pen = np.ones(p)
    pen[7] = 0.0
    kw = dict(lmda_path_size=30, early_exit=False, tol=1e-9, penalty=pen)
    on, off = on_off(monkeypatch, X, lambda Xd: ad.grpnet(Xd, ad.glm.gaussian(y), **kw))
    assert_identical(on, off, state_too=True)
    assert on.counters["n_sweeps_filtered"] > 0
