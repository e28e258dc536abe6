"""adelie_amd.bcd on the device against beta* = h* v / ((q + l2) h* + l1), h* the root of phi found by bisection in numpy
longdouble down to the last bit of h: plain, and independent of Newton.  q + l2 is formed in the working dtype, as the kernel and
the reference form it, so beta* is the exact solution of the problem the kernel is given."""
import functools

import numpy as np
import pytest

import adelie_amd as ad

gpu = pytest.mark.gpu
LD = np.longdouble
SOLVERS = ["newton", "newton_abs"]
TOL = {"float64": 1e-12, "float32": 1e-6}
# kernels_bcd.hip, bcd_lds_max_d<T>(): the largest d whose q + l2 and v are staged in LDS; one more is read from global memory
LDS_MAX_D = {"float64": 10176, "float32": 20352}
TEAM, WAVE, BLOCK = [1, 3, 4, 5, 64], [65, 130, 1024], [1025, 3000]
# max |beta - beta*| of the oracle's float64 group update (the same Newton rule from h = 0, summed in index order, tol 1e-12)
# over every float64 input of this file, as test_oracle_stays_inside_the_bound measures it on the CPU: 4.06e-13 (on the batch of
# d = 5; 9.4e-15 on the mixed batch, 2.5e-15 at d = 10177): what the stopping rule leaves, not rounding.  The kernel may be MARGIN
# times as far from beta*, which covers the different order of its sums; float32 stops at a tol 1e6 times larger and gets that
# ratio on top.
ORACLE_ERR = 4.1e-13
MARGIN = 4


def lengths(dtype):
    return TEAM + WAVE + BLOCK + [LDS_MAX_D[dtype] + 1]


@functools.lru_cache(maxsize=None)
def batch(d, dtype):
    """B seeded problems of length d with a root to find: 17 in the team tier (a last wavefront with one team of four), 3 beyond."""
    B = 17 if d <= 64 else 3
    rng = np.random.default_rng(d)
    quad = rng.uniform(0.5, 2.0, (B, d))
    linear = rng.normal(size=(B, d))
    l1 = rng.uniform(0.2, 0.8, B) * np.linalg.norm(linear, axis=1)
    l2 = rng.uniform(0.0, 0.5, B)
    return tuple(np.ascontiguousarray(a, dtype=dtype) for a in (quad, linear, l1, l2))


@functools.lru_cache(maxsize=None)
def mixed(dtype):
    """16 problems of length 5 (teams of 8 lanes, 8 to a wavefront) whose neighbours differ in kind:
    0 ||v|| <= l1,  1 l1 = 0,  2 an easy root,  3 quad over 1e-8 .. 1e4 with a wide bracket,  4 zeros in quad + l2, ||v_S|| < l1."""
    rng = np.random.default_rng(5)
    kinds = np.arange(16) % 5
    quad = rng.uniform(0.5, 2.0, (16, 5))
    linear = rng.normal(size=(16, 5))
    norm = np.linalg.norm(linear, axis=1)
    l1, l2 = 0.5 * norm, np.full(16, 0.1)
    l1[kinds == 0] = 1.5 * norm[kinds == 0]
    l1[kinds == 1] = 0.0
    quad[kinds == 3] = np.geomspace(1e-8, 1e4, 5)
    linear[kinds == 3] = [0.2, -0.2, 0.2, 3.0, -2000.0]  # (the root is near 1.6, the bracket [0, 2e7])
    l1[kinds == 3], l2[kinds == 3] = 0.5, 0.0
    quad[kinds == 4, :2] = 0.0
    l1[kinds == 4] = 0.5 * np.linalg.norm(linear[kinds == 4, 2:], axis=1)
    linear[kinds == 4, :2] *= 0.25 * l1[kinds == 4, None] / np.linalg.norm(linear[kinds == 4, :2], axis=1)[:, None]
    l2[kinds == 4] = 0.0
    return tuple(np.ascontiguousarray(a, dtype=dtype) for a in (quad, linear, l1, l2)) + (kinds,)


def phi(h, a, v, l1):
    return np.sum((v / (a * h + l1)) ** 2) - 1


def beta_star(q, v, l1, l2):
    a, v, l1 = (q + l2).astype(LD), v.astype(LD), LD(l1)
    if np.sqrt(np.sum(v * v)) <= l1:
        return np.zeros(q.size, dtype=LD)
    if l1 <= 0:
        return v / a
    lo, hi = LD(0), LD(1)
    while phi(hi, a, v, l1) > 0:
        hi *= 2
    while True:
        mid = lo + (hi - lo) / 2
        if mid == lo or mid == hi:
            break
        lo, hi = (mid, hi) if phi(mid, a, v, l1) > 0 else (lo, mid)
    return lo * v / (a * lo + l1)


@functools.lru_cache(maxsize=None)
def stars(name, dtype):
    quad, linear, l1, l2 = (batch(name, dtype) if isinstance(name, int) else mixed(dtype))[:4]
    return [beta_star(*p) for p in zip(quad, linear, l1, l2)]


def check(out, k, q, v, l1, l2, star, dtype):
    """The four assertions on problem k of a result."""
    beta, iters = np.asarray(out["beta"][k]), out["iters"][k]
    tol, eps, d = TOL[dtype], float(np.finfo(dtype).eps), q.size
    assert beta.dtype == np.dtype(dtype) and beta.shape == q.shape
    a = q + l2
    if np.sqrt(np.sum(v.astype(LD) ** 2)) <= l1:
        assert iters == 0 and not beta.any()
        return
    if l1 <= 0:
        assert iters == 0 and np.array_equal(beta.view(np.uint8), (v / a).view(np.uint8))
        return
    # stationarity: the solve stops with |t - 1| <= tol for its own t, whose sum of d terms of 9 roundings each is off by at most
    # (d + 9) eps, ||beta|| = h sqrt(t) with beta's own roundings (another 7 eps), and |h phi'(h)| <= 2 t
    h = np.sqrt(np.sum(beta.astype(LD) ** 2))
    slack = 2 * tol + (d + 16) * eps
    assert abs(phi(h, a.astype(LD), v.astype(LD), LD(l1))) <= slack, (k, float(phi(h, a.astype(LD), v.astype(LD), LD(l1))))
    resid = beta.astype(LD) * (a.astype(LD) * h + LD(l1)) - h * v.astype(LD)
    assert np.all(np.abs(resid) <= slack * h * np.abs(v.astype(LD))), k
    err = float(np.max(np.abs(beta.astype(LD) - star)))
    assert err <= MARGIN * ORACLE_ERR * (tol / TOL["float64"]), (k, err)


def check_all(out, quad, linear, l1, l2, star, dtype):
    assert out["iters"].dtype == np.int64 and out["iters"].shape == (len(quad),)
    for k in range(len(quad)):
        check(out, k, quad[k], linear[k], l1[k], l2[k], star[k], dtype)


def test_oracle_stays_inside_the_bound(oracle):
    worst = 0.0
    for name in lengths("float64") + ["mixed"]:
        quad, linear, l1, l2 = (batch(name, "float64") if isinstance(name, int) else mixed("float64"))[:4]
        for q, v, a, b, star in zip(quad, linear, l1, l2, stars(name, "float64")):
            x, _ = oracle.bcd_newton(q, v, a, b, tol=1e-12, max_iters=100000)
            worst = max(worst, float(np.max(np.abs(x.astype(LD) - star))))
    print(f"oracle: max |beta - beta*| = {worst:.3e}")
    assert worst <= ORACLE_ERR


@gpu
@pytest.mark.parametrize("dtype", list(TOL))
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("d", TEAM + WAVE + BLOCK + ["past_lds"])
def test_rectangular(hip, d, solver, dtype):
    d = LDS_MAX_D[dtype] + 1 if d == "past_lds" else d
    quad, linear, l1, l2 = batch(d, dtype)
    out = ad.bcd.solve_many(quad=quad, linear=linear, l1=l1, l2=l2, tol=TOL[dtype], solver=solver)
    assert out["beta"].shape == quad.shape and out["time_elapsed"] > 0
    check_all(out, quad, linear, l1, l2, stars(d, dtype), dtype)


@gpu
@pytest.mark.parametrize("dtype", list(TOL))
@pytest.mark.parametrize("solver", SOLVERS)
def test_ragged_and_bit_reproducible(hip, solver, dtype):
    """Every length in one call; then one problem of each tier alone and in first, middle and last place: the same bits."""
    ds = lengths(dtype)
    rows = [[a[1] for a in batch(d, dtype)] for d in ds]
    quad, linear, l1, l2 = ([r[i] for r in rows] for i in range(4))
    kw = dict(tol=TOL[dtype], solver=solver)
    out = ad.bcd.solve_many(quad=quad, linear=linear, l1=l1, l2=l2, **kw)
    assert isinstance(out["beta"], list) and [b.size for b in out["beta"]] == ds
    check_all(out, quad, linear, l1, l2, [stars(d, dtype)[1] for d in ds], dtype)
    for k in (ds.index(5), ds.index(130), ds.index(3000), len(ds) - 1):
        alone = ad.bcd.solve(quad=quad[k], linear=linear[k], l1=l1[k], l2=l2[k], **kw)
        assert alone["iters"] == out["iters"][k] and np.array_equal(alone["beta"].view(np.uint8), out["beta"][k].view(np.uint8))
        for place in (0, len(ds) // 2, len(ds) - 1):
            order = [i for i in range(len(ds)) if i != k]
            order.insert(place, k)
            again = ad.bcd.solve_many(quad=[quad[i] for i in order], linear=[linear[i] for i in order],
                                      l1=np.array(l1)[order], l2=np.array(l2)[order], **kw)
            assert again["iters"][place] == alone["iters"]
            assert np.array_equal(again["beta"][place].view(np.uint8), alone["beta"].view(np.uint8))


@gpu
@pytest.mark.parametrize("dtype", list(TOL))
@pytest.mark.parametrize("solver", SOLVERS)
def test_neighbours_of_different_kinds(hip, solver, dtype):
    quad, linear, l1, l2, kinds = mixed(dtype)
    h_min = ad.bcd.root_lower_bound(quad=quad[3], linear=linear[3], l1=l1[3])
    assert ad.bcd.root_upper_bound(quad=quad[3], linear=linear[3], l1=l1[3]) - h_min > 0.1
    out = ad.bcd.solve_many(quad=quad, linear=linear, l1=l1, l2=l2, tol=TOL[dtype], solver=solver)
    check_all(out, quad, linear, l1, l2, stars("mixed", dtype), dtype)
    assert np.all((out["iters"] == 0) == (kinds < 2))


@gpu
@pytest.mark.parametrize("dtype", list(TOL))
def test_device_tensors(hip, dtype):
    import torch

    quad, linear, l1, l2 = batch(130, dtype)
    host = ad.bcd.solve_many(quad=quad, linear=linear, l1=l1, l2=l2, tol=TOL[dtype])
    q_t, v_t = torch.from_numpy(quad).to("cuda"), torch.from_numpy(linear).to("cuda")
    dev = ad.bcd.solve_many(quad=q_t, linear=v_t, l1=l1, l2=l2, tol=TOL[dtype])
    assert dev["beta"].is_cuda and dev["beta"].shape == q_t.shape
    assert np.array_equal(dev["beta"].cpu().numpy().view(np.uint8), host["beta"].view(np.uint8))
    assert np.array_equal(dev["iters"], host["iters"])
    assert np.array_equal(q_t.cpu().numpy(), quad) and np.array_equal(v_t.cpu().numpy(), linear)
