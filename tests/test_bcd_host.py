"""adelie_amd.bcd without a device: the four scalar routines against their closed forms in numpy longdouble, the existence check
of root() and the solver names that are out of scope."""
import numpy as np
import pytest

import adelie_amd as ad

LD = np.longdouble
bcd = ad.bcd
# (quad, linear, l1); the third has a zero in quad with ||linear_S|| < l1, the fourth is a single value
INPUTS = [
    ([1.0, 2.0, 0.5], [1.0, -2.0, 0.5], 0.7),
    ([0.3, 4.0, 1.5, 2.5, 0.9], [0.2, 3.0, -1.0, 0.1, 2.0], 1.3),
    ([0.0, 2.0, 1.0, 0.5], [0.3, 1.0, -2.0, 0.7], 0.9),
    ([2.0], [3.0], 1.0),
]


def as_ld(*a):
    return [np.asarray(x, dtype=LD) for x in a]


def phi_ld(h, quad, linear, l1):
    q, v = as_ld(quad, linear)
    return np.sum(v ** 2 / (q * LD(h) + LD(l1)) ** 2) - 1


@pytest.mark.parametrize("quad, linear, l1", INPUTS)
def test_scalar_routines_against_closed_forms(quad, linear, l1):
    q64, v64 = np.array(quad), np.array(linear)
    q, v = as_ld(quad, linear)
    for h in (0.0, 0.4, 3.0):
        assert bcd.root_function(h, quad=q64, linear=v64, l1=l1) == pytest.approx(float(phi_ld(h, quad, linear, l1)), rel=1e-13, abs=1e-14)
    # lower bound: the larger root of a h^2 + 2 b h + c (Cauchy-Schwarz on phi), clipped at 0
    a, b = np.sum(q * q), LD(l1) * np.sum(q)
    c = LD(l1) ** 2 * q.size - np.sum(np.abs(v)) ** 2
    lower = bcd.root_lower_bound(quad=q64, linear=v64, l1=l1)
    assert lower == pytest.approx(float(max((-b + np.sqrt(max(b * b - a * c, LD(0)))) / a, LD(0))), rel=1e-13)
    assert lower >= 0 and phi_ld(lower, quad, linear, l1) >= -1e-14
    # upper bound: ||v / q|| over the non-zero entries, inflated by the share of l1 that the zero entries use up
    nz = q > 0
    upper = np.sqrt(np.sum((v[nz] / q[nz]) ** 2) / (1 - np.sum(v[~nz] ** 2) / LD(l1) ** 2))
    assert bcd.root_upper_bound(quad=q64, linear=v64, l1=l1) == pytest.approx(float(upper), rel=1e-13)
    assert phi_ld(upper, quad, linear, l1) <= 1e-14
    # zero_tol: entries up to it leave the sum (when there is one), but only true zeros use up l1
    big = q > 0.6 if q.min() <= 0.6 else nz
    upper_tol = np.sqrt(np.sum((v[big] / q[big]) ** 2) / (1 - np.sum(v[~nz] ** 2) / LD(l1) ** 2))
    assert bcd.root_upper_bound(quad=q64, linear=v64, l1=l1, zero_tol=0.6) == pytest.approx(float(upper_tol), rel=1e-13)
    beta, l2 = v / 3, 0.25
    obj = np.sum(q * beta ** 2) / 2 - np.sum(v * beta) + LD(l1) * np.sqrt(np.sum(beta ** 2)) + LD(l2) / 2 * np.sum(beta ** 2)
    assert bcd.objective(beta.astype(np.float64), quad=q64, linear=v64, l1=l1, l2=l2) == pytest.approx(float(obj), rel=1e-13)


def test_root_does_not_exist():
    quad, linear = np.array([0.0, 2.0, 1.0]), np.array([0.3, 1.0, -2.0])
    assert bcd.root(quad=quad, linear=linear, l1=3.0) == {"root": None, "iters": 0}  # ||v|| <= l1
    assert bcd.root(quad=quad, linear=linear, l1=0.2) == {"root": None, "iters": 0}  # ||v_S|| >= l1


@pytest.mark.parametrize("solver", ["newton_brent", "brent", "ista", "fista", "fista_adares", "newton_abs_debug"])
@pytest.mark.parametrize("entry", ["solve", "solve_many", "root"])
def test_solvers_out_of_scope(entry, solver):
    quad, linear = np.array([1.0, 2.0]), np.array([1.0, -2.0])
    kw = dict(quad=quad[None], linear=linear[None], l2=0.0) if entry == "solve_many" else dict(quad=quad, linear=linear)
    if entry == "solve":
        kw["l2"] = 0.0
    with pytest.raises(NotImplementedError, match='"newton" and "newton_abs"'):
        getattr(bcd, entry)(l1=0.5, solver=solver, **kw)


def test_empty_batch_needs_no_native_call():
    out = bcd.solve_many(quad=np.empty((0, 3)), linear=np.empty((0, 3)), l1=0.5, l2=0.0)
    assert out["beta"].shape == (0, 3) and out["iters"].shape == (0,) and out["iters"].dtype == np.int64
    out = bcd.solve_many(quad=[], linear=[], l1=0.5, l2=0.0)
    assert out["beta"] == [] and out["iters"].shape == (0,) and out["time_elapsed"] == 0.0
