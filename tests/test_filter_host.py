"""The bound behind the filtered invariance sweep, restated in numpy: with xs_j = column j rounded to float32 and
e_j = ||x_j - xs_j||_2, the two sweeps' values differ by at most (e_j + 4 n 2^-53 ||xs_j||_2) ||v||_2 (1 + 1e-6) -- the first
term is Cauchy-Schwarz on (x_j - xs_j) . v, the second covers the rounding of the two f64 accumulations (each at most
n 2^-53 sum |x_i v_i| <= n 2^-53 ||x|| ||v||, doubled for margin)."""
import os
import shutil
import subprocess

import numpy as np
import pytest


def sweep_pair(X, v):
    """(exact, shadow) as sequential f64 accumulations, like a kernel's (any summation order obeys the same bound)."""
    Xs = X.astype(np.float32).astype(np.float64)
    return X.T @ v, Xs.T @ v, Xs


def bound(X, Xs, v):
    e = np.sqrt(((X - Xs) ** 2).sum(axis=0))
    return (e + 4 * X.shape[0] * 2.0 ** -53 * np.sqrt((Xs ** 2).sum(axis=0))) * np.sqrt((v ** 2).sum()) * (1 + 1e-6)


@pytest.mark.parametrize("n,p,scale", [(1, 7, 1.0), (300, 50, 1.0), (5000, 20, 1e-3), (777, 33, 1e30), (500, 10, 1e-40)])
def test_bound_holds_on_random_designs(n, p, scale):
    rng = np.random.RandomState(n + p)
    X = rng.normal(size=(n, p)) * scale
    v = rng.normal(size=n) * rng.uniform(size=n)
    exact, shadow, Xs = sweep_pair(X, v)
    # the reference difference in extended precision, so that the test's own rounding does not enter
    ref = np.array([float(np.sum((X[:, j].astype(np.longdouble) - Xs[:, j].astype(np.longdouble)) * v.astype(np.longdouble)))
                    for j in range(p)])
    b = bound(X, Xs, v)
    assert (np.abs(ref) <= b).all()
    assert (np.abs(exact - shadow) <= b).all()


def test_bound_holds_when_v_is_aligned_with_the_rounding_error():
    rng = np.random.RandomState(0)
    n, p = 4000, 6
    X = rng.normal(size=(n, p))
    Xs = X.astype(np.float32).astype(np.float64)
    v = X[:, 2] - Xs[:, 2]          # Cauchy-Schwarz is tight for column 2: |(x - xs) . v| = e ||v||
    exact, shadow, _ = sweep_pair(X, v)
    b = bound(X, Xs, v)
    d = np.abs(exact - shadow)
    assert (d <= b).all()
    e2 = np.sqrt(((X[:, 2] - Xs[:, 2]) ** 2).sum())
    assert d[2] >= 0.999 * e2 * np.sqrt((v ** 2).sum())   # the adversarial column really sits at the bound
    # a group's bound is the 2-norm of its columns' bounds (triangle inequality on the block norm)
    assert abs(np.sqrt((exact ** 2).sum()) - np.sqrt((shadow ** 2).sum())) <= np.sqrt((b ** 2).sum())


def test_host_logic_under_sanitizers(tmp_path):
    """The threshold rule, the list of unpenalized columns and the follow-up of a sweep's flags (adelie_amd/csrc/filter_host.hpp,
    what the solver calls) as a stand-alone program under the address and undefined-behaviour sanitizers, on the CPU."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is required (the oracle needs one as well)"
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "filter_host_main.cpp")
    exe = str(tmp_path / "filter_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "filter_host: ok" in out.stdout, out.stdout + out.stderr
