"""The 16-bit shadow copy (q15) of the filtered invariance sweep on the CPU: the encoding and its bound restated in numpy, and
the rule that picks a design's kind (adelie_amd/csrc/shadow_kind_host.hpp) as a stand-alone program under sanitizers.

Encoding: s_j = max_i |x_ij| / 32767, q_ij = clamp(rint(x_ij * (32767 / max_i |x_ij|)), +-32767), the copy is xs_ij = s_j q_ij.
Bound: the two sweeps' values differ by at most (e_j + (4 n + 8) 2^-53 ||xs_j||) ||v|| (1 + 1e-6), e_j = ||x_j - xs_j||."""
import os
import shutil
import subprocess

import numpy as np
import pytest


def q15_encode(X):
    """(q as float64 integers, s) of the columns of X; a zero column, and one whose scale would be subnormal or whose
    32767 / max overflows, has s = 0 and q = 0."""
    m = np.abs(X).max(axis=0)
    with np.errstate(divide="ignore", over="ignore"):
        inv = np.where(m > 0, 32767.0 / m, 0.0)
    s = m / 32767.0
    dead = ~np.isfinite(inv) | ~(s >= np.finfo(np.float64).tiny)   # (no subnormal scale: such a column is stored as zeros)
    inv[dead] = 0.0
    s[dead] = 0.0
    q = np.clip(np.rint(X * inv), -32767.0, 32767.0)
    return q, s


def q15_err_nrm(X):
    """(e_j, ||xs_j||) with the sums taken on x / s_j, so that a column of huge entries does not overflow them."""
    q, s = q15_encode(X)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.where(s > 0, (X - s * q) / s, 0.0)
    e = np.where(s > 0, s * np.sqrt((d ** 2).sum(axis=0)), np.sqrt(X.shape[0]) * np.abs(X).max(axis=0))
    return e, s * np.sqrt((q ** 2).sum(axis=0))


def q15_bounds(X, v):
    e, nx = q15_err_nrm(X)
    return (e + (4 * X.shape[0] + 8) * 2.0 ** -53 * nx) * np.sqrt((v ** 2).sum()) * (1 + 1e-6)


@pytest.mark.parametrize("n,p,scale", [(1, 7, 1.0), (300, 50, 1.0), (5000, 20, 1e-3), (777, 33, 1e30), (500, 10, 1e-300)])
def test_q15_bound_holds_on_random_designs(n, p, scale):
    rng = np.random.RandomState(n + p)
    X = rng.normal(size=(n, p)) * scale
    v = rng.normal(size=n) * rng.uniform(size=n)
    q, s = q15_encode(X)
    assert (np.abs(q) <= 32767).all() and (np.abs(q).max(axis=0) == 32767).all()
    shadow = (q.T @ v) * s                     # as the kernel: f64 accumulation of q . v, one multiplication by s_j
    exact = X.T @ v
    ld = np.longdouble
    ref = np.array([float(np.sum((X[:, j].astype(ld) - ld(s[j]) * q[:, j].astype(ld)) * v.astype(ld))) for j in range(p)])
    b = q15_bounds(X, v)
    assert (np.abs(ref) <= b).all()
    assert (np.abs(exact - shadow) <= b).all()


def test_q15_error_figures_of_gaussian_zero_one_and_heavy_tailed_columns():
    rng = np.random.RandomState(1)
    n = 100000
    X = np.empty((n, 4))
    X[:, 0] = rng.normal(size=n)
    X[:, 1] = (rng.uniform(size=n) < 0.3).astype(np.float64)
    X[:, 2] = 0.0
    X[:, 3] = rng.standard_t(3, size=n)
    e, nx = q15_err_nrm(X)
    assert 2e-5 < e[0] / nx[0] < 6e-5          # a Gaussian column: about 4e-5, far inside 2^-11
    assert e[1] == 0.0 and nx[1] == np.sqrt(X[:, 1].sum())   # 0/1: fl(fl(1 / 32767) * 32767) = 1, the copy is the column
    assert e[2] == 0.0 and nx[2] == 0.0
    assert e[3] / nx[3] > 2.0 ** -11 / 4       # t_3 at this n: the maximum is tens of standard deviations
    v = rng.normal(size=n)
    q, s = q15_encode(X)
    assert (np.abs(X.T @ v - (q.T @ v) * s) <= q15_bounds(X, v)).all()


def test_kind_rule_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is required (the oracle needs one as well)"
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "shadow_kind_main.cpp")
    exe = str(tmp_path / "shadow_kind")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "shadow_kind: ok" in out.stdout, out.stdout + out.stderr
