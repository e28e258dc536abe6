"""fp_term of the 16-bit shadow sweep (ShadowView::fp_term, kernels.hpp; derived in kernels_filter.hip) against the arithmetic
of shadow_sweep_kernel<ShadowQ15> restated in numpy, no GPU.

The kernel keeps q . v in f64: per lane one fma per row, rows ascending (the pipelined body loop issues its loads in another
order than the plain loop did and changes no fma), the shuffle ladder over a wave, the four waves added in order, and one
multiplication by the column's scale.  n = 4096 is one workgroup with two trips of 2048 rows: lane t takes rows 8 t .. 8 t + 7
of each.  The fma is emulated exactly: the product of a 16-bit integer and a double as two doubles (Dekker), then the sum of
three doubles rounded once through a round-to-odd intermediate (Boldo and Melquiond, "Emulation of FMA and correctly rounded
sums: proved algorithms using rounding to odd", 2008).  References are exact sums (exact_dot)."""
import math
from fractions import Fraction

import numpy as np

from test_shadow_kind_host import q15_encode, q15_err_nrm

U = 2.0 ** -53


def fp_term(n):
    return (4.0 * n + 8.0) * 1.1102230246251565e-16   # ShadowView::fp_term() of the q15 kind


def exact_dot(a, b):
    """sum a_i b_i as a Fraction: every product split into two doubles that add up to it exactly, all of them through fsum
    (exact up to its one final rounding, 2^-53 of the sum itself: the callers compare against bounds of n 2^-53 and more times
    the sum of the |a_i b_i|)."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    # both scaled to a largest entry in [0.5, 1): neither the products nor the splitting constant overflow
    ea = np.frexp(np.abs(a).max() or 1.0)[1]
    eb = np.frexp(np.abs(b).max() or 1.0)[1]
    a2, b2 = np.ldexp(a, -ea), np.ldexp(b, -eb)
    hi, lo = two_prod(a2, b2)
    tiny = (np.abs(hi) < 2.0 ** -900) & (a2 != 0) & (b2 != 0)   # (`lo` could lose bits to underflow there: those exactly)
    total = Fraction(math.fsum(hi[~tiny].tolist() + lo[~tiny].tolist()))
    for x, y in zip(a2[tiny].tolist(), b2[tiny].tolist()):
        total += Fraction(x) * Fraction(y)
    return total * Fraction(2) ** (int(ea) + int(eb))


def two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def two_prod(a, b):
    c = 134217729.0   # 2^27 + 1
    hi = a * b
    ah = (a * c) - ((a * c) - a)
    al = a - ah
    bh = (b * c) - ((b * c) - b)
    bl = b - bh
    return hi, ((ah * bh - hi) + ah * bl + al * bh) + al * bl


def round_to_odd_sum(a, b):
    """a + b rounded to odd: the exact sum when it is a double, else the neighbour of it with an odd last bit"""
    s, e = two_sum(a, b)
    bits = s.view(np.int64)
    fix = (e != 0) & ((bits & 1) == 0)
    # an even s off the exact sum: the odd neighbour lies on the side of the error
    toward = np.where(e > 0, np.inf, -np.inf)
    return np.where(fix, np.nextafter(s, toward), s)


def fma(a, b, c):
    """round(a b + c) with one rounding, elementwise (no overflow or underflow at the magnitudes used here)"""
    ph, pl = two_prod(a, b)
    uh, ul = two_sum(pl, c)
    th, tl = two_sum(ph, uh)
    return th + round_to_odd_sum(tl, ul)


def test_fma_emulation_is_the_correctly_rounded_one():
    rng = np.random.RandomState(3)
    a = rng.randint(-32767, 32768, size=4000).astype(np.float64)
    b = rng.normal(size=4000) * 10.0 ** rng.randint(-8, 8, size=4000)
    c = -a * b * (1 + rng.normal(size=4000) * 10.0 ** rng.randint(-17, 0, size=4000))   # cancellation of every depth
    got = fma(a, b, c)
    for x, y, z, g in zip(a.tolist(), b.tolist(), c.tolist(), got.tolist()):
        assert g == float(Fraction(x) * Fraction(y) + Fraction(z))   # (float(Fraction) rounds to nearest even)


def kernel_value(q, scale, V):
    """The shadow's value of one column (q: 4096 integers as doubles, its scale) for every row of V (draws x 4096)"""
    n = q.shape[0]
    assert n == 4096
    d = V.shape[0]
    acc = np.zeros((d, 256))
    for trip in range(2):
        rows = trip * 2048 + 8 * np.arange(256)
        for e in range(8):
            acc = fma(np.broadcast_to(q[rows + e], (d, 256)).copy(), V[:, rows + e].copy(), acc)
    x = acc.reshape(d, 4, 64).copy()
    for off in (32, 16, 8, 4, 2, 1):   # wave_sum: x += shfl_down(x, off); lane 0 of each wave carries the sum
        x[:, :, :64 - off] = x[:, :, :64 - off] + x[:, :, off:]
    s = np.zeros(d)
    for w in range(4):
        s = s + x[:, w, 0]
    return s * scale


def test_bound_with_fp_term_holds_for_the_kernels_arithmetic():
    n, draws = 4096, 2000
    rng = np.random.RandomState(11)
    x = rng.normal(size=(n, 1))
    q, s = q15_encode(x)
    err, nrm = q15_err_nrm(x)
    q, s, err, nrm = q[:, 0], float(s[0]), float(err[0]), float(nrm[0])
    xs = q * s
    V = rng.normal(size=(draws, n))
    V[1::2] = np.where(q >= 0, 1.0, -1.0) * rng.uniform(0.5, 2.0, size=(draws // 2, n))   # every other draw: signs aligned with q
    got = kernel_value(q, s, V)
    ft = fp_term(n)
    worst_copy = worst_true = 0.0
    for k in range(draws):
        v = V[k]
        vnorm = math.sqrt(math.fsum((v * v).tolist()))   # (v * v rounds each square: 2^-53 relative, far inside the slack below)
        g = Fraction(float(got[k]))
        d_copy = abs(g - exact_dot(xs, v))
        d_true = abs(g - exact_dot(x[:, 0], v))
        b_copy = Fraction(ft) * Fraction(nrm) * Fraction(vnorm)
        b_true = (Fraction(err) + Fraction(ft) * Fraction(nrm)) * Fraction(vnorm)
        assert d_copy <= b_copy and d_true <= b_true, (k, float(d_copy), float(b_copy), float(d_true), float(b_true))
        worst_copy = max(worst_copy, float(d_copy / b_copy))
        worst_true = max(worst_true, float(d_true / b_true))
    print("largest error / bound over %d draws: %.3g on the copy (fp_term alone), %.3g on the column" % (draws, worst_copy, worst_true))
    # the derivation needs (2 n + 1) u nrm for the body and the scale: the kernel's own share stays inside half of fp_term
    assert worst_copy <= 0.5


def test_fp_term_is_small_against_the_quantisation_error():
    """A Gaussian column: fp_term nrm stays below err / 8 at the test's n and at the headline's, so the filter opens no more
    columns for floating-point reasons than for the copy's own error."""
    rng = np.random.RandomState(5)
    for n in (4096, 100000):
        x = rng.normal(size=(n, 1))
        err, nrm = q15_err_nrm(x)
        assert fp_term(n) * nrm[0] < err[0] / 8
        assert 1e-5 * nrm[0] < err[0] < 1e-4 * nrm[0]
