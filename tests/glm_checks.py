"""The GLM family kernels (adelie_amd/csrc/kernels_glm.hip), one launch at a time, against plain references (no GPU needed to
import).

A *call* is one ``adelie_hip_glm_piece_test``: one of the thirteen launchers the IRLS wrapper runs (PREPARE, WEIGHTS, FINISH,
NULL_STEP, GRADIENT, LOSS, LOSS2, MULTI_LOSS2, SET_ETA, DOT_DIFF, REL_CHANGE, GATHER, SCATTER) on the caller's arrays.  This module
holds the inputs (built from named seeds), the references, ``device_call``, ``emulate_call`` -- a plain numpy model of every kernel
in the value type, which follows the kernels' summation order and takes an optional planted defect -- and the derivation of every
bound.  tests/test_gpu_glm_pieces.py runs the checks on the device, tests/test_glm_checks_host.py runs the same checks on the
model and on the planted defects.  u = 2^-53 / 2^-24 is the unit roundoff, gamma_m = m u / (1 - m u).

Exact leg (Gaussian kind, SET_ETA, DOT_DIFF, WEIGHTS with hess_sum = 2^10, GATHER, SCATTER).  Inputs are small integers.  The
weight of element i is 2^c(i), c(i) counting the position classes i belongs to (last lane of a wave, last thread of a workgroup,
last thread of the grid, second stride trip, the tail element, odd index), so elements of different classes contribute
differently; every term of a sum is non-zero.  The checker asserts sum |term| < 2^24 (in units of 2^-10 for WEIGHTS), so every
product and partial sum is exact in float32 and float64 in any order, fused or not, and outputs are compared bit for bit with an
int64 reference.

Rounding leg (logit, probit, Poisson, multinomial through every launcher that takes a kind; also the Gaussian member).  The
reference is the kernel's stated formula -- glm_binomial.ipp:37-99 (logit), :100-173 (probit), glm_poisson.ipp:14-44,
glm_multinomial.ipp:21-87, glm_base.ipp:23-37 (the raised Hessian) as restated in the kernel's comments -- evaluated operation for
operation by ``Arith`` in mpmath at 60 digits.  Arith carries with every intermediate value v a bound e on |computed - v| in the
value type, by the standard model: an arithmetic operation returns its exact result times (1 + d), |d| <= u, plus at most the
smallest subnormal; a call of exp, log or erf returns the exact function of its (already perturbed) argument times (1 + d),
|d| <= A ulp = 2 A u.  Errors of the arguments are propagated exactly as the operation conditions them: a sum adds them, a product
weighs them by the other factor, a quotient divides by |b| - e_b, exp multiplies by expm1(e), log adds -log1p(-e / v), erf the
largest derivative over the argument's interval.  So the factor c / (1 - c) of the probit member's 1 - c, and the absolute term of
the logit member's log(1 + exp(-|e|)), are in the bound because the formula has them, not by a flat tolerance; where a
denominator or a log argument could reach zero within its bound, Arith refuses the input (that is the band of eta left out of
both legs).  An operation on exact operands whose exact result is representable in the value type is exact (a rounding that cannot
happen is not charged): integers stay exact, and a Hessian that is exactly zero is known to be.  A fused multiply-add rounds once
where the model rounds twice, so it stays inside the bound.

A_ULP = 4 for exp, log and erf in both types.  No accuracy table of the HIP math functions was found under the ROCm installation,
so this is the issue's fallback and an ASSUMPTION NOBODY MEASURED HERE.  An output outside its bound is a kernel bug until shown
otherwise: compare it with ``emulate_call`` (the formula in the value type on the host) before touching A.

mpmath is slow, so it only ever sees a base vector of NBASE = 131 elements (NBASE_MULTI = 37 rows for the row-coupled kernels)
per kind and type; it holds eta = 0, +-tiny and both ends of the range besides random values.  The n of N_LIST index it as
i % NBASE: elementwise outputs of a call with any n must equal, bit for bit, the base call's device outputs at i % NBASE (the
arithmetic per element is the same, and the base call is what mpmath judged), and a reduction is checked against the exact sum of
the tiled reference terms t_j with

    |S - sum t| <= (1 + gamma_m) sum e_j + gamma_m sum |t_j|,   m = ceil(n / 65536) + 6 + 4 + 6 + 4,

counted from the code: a thread adds ceil(n / 65536) terms, the wave shuffle has 6 steps, a workgroup adds its 4 waves, and the
final reduce over the 256 partials does the 6 + 4 again.  Every reduction is run twice and must repeat its bits.

Ranges of eta on the rounding leg (RANGES, printed by the tests): wide enough to reach both tails, narrow enough that every bound
stays a small multiple of u relative to the larger of the value and 1: the probit member's c / (1 - c) stays below 4e6 in
float64 (|eta| <= 5) and below 800 in float32 (|eta| <= 3).

Decision leg.  Inputs where a branch decides.  Most go through the same Arith reference, which then yields e = 0 (exact
equality) wherever the decision makes the result exact: the raise to hessian_min (rows with w = 0, rows whose Hessian is exactly
zero because resid is exactly w y, the logit and multinomial `w <= 0` guards, pre-filled Hessians of the CALLBACK and COX kinds that
are zero or negative) gives hess == hessian_min, and z and irls_y are additionally compared bit for bit with resid / hessian_min
and z + eta - off in numpy.  Arith refuses a Hessian whose sign its bound does not decide.  Probit clamps: at |eta| >= 12
(float64) / 8 (float32) the distance of erf(eta / sqrt 2) to +-1 is below 2^-20 ulp (3.5e-33 < 2^-73; 1.2e-15 < 2^-44; checked on the
host with mpmath), so c is exactly 0 or 1 on any libm that saturates, and the reference is the formula with c set to 0 or 1 and
the clamps by the largest finite value applied; the exp of the density keeps its A ulp and its conditioning.  Multinomial rows
with eta near +-700 / +-80 and rows of equal classes go through the shifted formula.  Where the value type overflows on the way
(logit at eta = +-800 / +-100, Poisson loss at eta = -inf or -1e300 / -1e30) the mpmath model does not apply and the expected
value is written out in numpy in the value type and compared bit for bit.  REL_CHANGE is compared bit for bit with the same
expression in numpy: -, / and fabs are IEEE-exact and the library is built with -O3 and no fast-math flag (build.sh).

Planted defects (``emulate_call(..., defect=)``): 'drop_tail' (every grid-stride loop stops one element early), 'skip_trip2'
(no thread takes a second stride trip), 'swap_acc' (accumulators 1 and 2 of WEIGHTS land in each other's slot), 'h0_lt'
(h0 <= 0 read as h0 < 0), 'raise_after_div' (z formed with the unraised Hessian), 'no_w_guard' (the logit and multinomial
denominators without T(w <= 0)), 'no_probit_clamp', 'no_shift' (multinomial without the max-shift), 'rel_no_reset', 'rel_nan_zero',
'row_major' (the multi-response arrays addressed [i K + k]).
"""
import ctypes as C
import functools

import mpmath
import numpy as np
from scipy.special import erf as sp_erf

from group_checks import DT_CODE, NP_TYPE, UNIT, _rng, bits, gamma, is_prefill, prefill

A_ULP = 4          # allowance per exp / log / erf call, in ulp: the issue's fallback, not measured (see above)
(GAUSSIAN, LOGIT, GAUSSIAN_IRLS, MULTINOMIAL, POISSON, PROBIT, CALLBACK, COX) = range(8)
KIND_NAME = {GAUSSIAN: "gaussian", LOGIT: "logit", GAUSSIAN_IRLS: "gaussian_irls", MULTINOMIAL: "multinomial", POISSON: "poisson",
             PROBIT: "probit", CALLBACK: "callback", COX: "cox"}
(M_PREPARE, M_WEIGHTS, M_FINISH, M_NULL, M_GRAD, M_LOSS, M_LOSS2, M_MLOSS2, M_SET_ETA, M_DOT, M_REL, M_GATHER, M_SCATTER) = range(13)
MODE_NAME = ("prepare", "weights", "finish", "null_step", "gradient", "loss", "loss2", "multi_loss2", "set_eta", "dot_diff",
             "rel_change", "gather", "scatter")
RB = RT = 256
STRIDE = RB * RT
N_LIST = (1, 63, 64, 65, 255, 256, 257, 2053, 65535, 65536, 65537, 131149)
# (nb, K) of the row-coupled kernels: every nb of N_LIST at some K, nb K <= 200 k, a second stride trip over rows at K = 2 and 3
MULTI_SHAPES = ((1, 1), (63, 2), (64, 3), (65, 7), (255, 7), (256, 1), (257, 2), (2053, 3), (2053, 7), (65535, 1), (65536, 2),
                (65537, 3), (131149, 1))
MOVE_CNT = (0, 1, 255, 256, 257, 1000)
NBASE, NBASE_MULTI = 131, 37
SENTINEL = 2.0 ** 120
HMIN = 1e-24       # configs.hessian_min's default
DEFECTS = ("drop_tail", "skip_trip2", "swap_acc", "h0_lt", "raise_after_div", "no_w_guard", "no_probit_clamp", "no_shift",
           "rel_no_reset", "rel_nan_zero", "row_major")
# eta on the rounding leg, per kind and type
RANGES = {(LOGIT, "f64"): 20.0, (LOGIT, "f32"): 10.0, (PROBIT, "f64"): 5.0, (PROBIT, "f32"): 3.0, (POISSON, "f64"): 8.0,
          (POISSON, "f32"): 4.0, (MULTINOMIAL, "f64"): 10.0, (MULTINOMIAL, "f32"): 4.0, (GAUSSIAN, "f64"): 8.0, (GAUSSIAN, "f32"): 8.0}
PROBIT_SAT = {"f64": 12.0, "f32": 8.0}
SHIFT_ETA = {"f64": 700.0, "f32": 80.0}
LOGIT_SAT = {"f64": 800.0, "f32": 100.0}
POISSON_HUGE = {"f64": -1e300, "f32": -1e30}
EXP_ZERO = {"f64": -800.0, "f32": -120.0}      # exp underflows to exactly zero (below -745.2 / -104)

POINTERS = ("y", "w", "wb", "eta", "resid", "off", "hess", "irls_resid", "irls_y", "wts", "cb_z", "b0v", "resid_prev", "eta_prev",
            "prev", "src", "idx", "dst", "sums")
OUTPUTS = {M_PREPARE: ("hess", "irls_resid", "irls_y"), M_WEIGHTS: ("wts", "irls_resid"), M_FINISH: ("eta", "resid"), M_NULL: (),
           M_GRAD: ("resid",), M_LOSS: (), M_LOSS2: (), M_MLOSS2: (), M_SET_ETA: ("eta",), M_DOT: (), M_REL: ("prev",),
           M_GATHER: ("dst",), M_SCATTER: ("dst",)}
NSUMS = {M_PREPARE: 1, M_WEIGHTS: 3, M_NULL: 2, M_LOSS: 1, M_LOSS2: 2, M_MLOSS2: 2, M_DOT: 1}

ctx = mpmath.mp.clone()
ctx.dps = 60
M = ctx.mpf


def device_call(hip, mode, dtype, a):
    """Runs one call on the device.  `a`: field name -> contiguous numpy array (written in place where the mode writes) or scalar;
    a['sums'] (16 values) is created when missing.  Returns info (8 values)."""
    from adelie_amd import _abi

    s = _abi.GlmPiece()
    s.dtype, s.mode, s.sentinel = DT_CODE[dtype], mode, SENTINEL
    if "sums" not in a:
        a["sums"] = prefill(dtype, 16)
    for k, v in a.items():
        if k in POINTERS:
            if v is None:
                continue
            assert v.dtype == (np.int32 if k == "idx" else NP_TYPE[dtype]) and v.flags.c_contiguous, k
            setattr(s, k, v.ctypes.data)
        else:
            setattr(s, k, v)
    info = np.full(8, -1, dtype=np.int64)
    hip.check(hip.fn("glm_piece_test")(C.byref(s), info.ctypes.data))
    return info


def copy_inputs(a):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in a.items()}


# ---- the kernels in numpy in the value type (the faithful model, and its planted defects) --------------------------------------
def _fmax(T):
    return T(np.finfo(T).max)


def np_cdf(T, x):
    return T(0.5) * (T(1) + sp_erf(x * T(0.70710678118654752440)).astype(T))


def np_pdf(T, x):
    return T(0.39894228040143267794) * np.exp(T(-0.5) * x * x)


def np_grad(T, kind, y, w, eta, defect=None):
    with np.errstate(all="ignore"):
        if kind == LOGIT:
            return w * (y - T(1) / (T(1) + np.exp(-eta)))
        if kind == POISSON:
            return w * (y - np.exp(eta))
        if kind == PROBIT:
            mx, c = _fmax(T), np_cdf(T, eta)
            a, b = T(1) / c, T(1) / (T(1) - c)
            if defect != "no_probit_clamp":
                a, b = np.fmin(a, mx), np.fmin(b, mx)
            return w * np_pdf(T, eta) * (y * a - (T(1) - y) * b)
        return w * (y - eta)


def np_loss_term(T, kind, y, e, defect=None):
    with np.errstate(all="ignore"):
        if kind == LOGIT:
            return ((e > 0).astype(T) - y) * e + np.log(T(1) + np.exp(-np.abs(e)))
        if kind == POISSON:
            return np.fmin(-e, _fmax(T)) * y + np.exp(e)
        if kind == PROBIT:
            mx, c = _fmax(T), np_cdf(T, e)
            a, b = np.log(c), np.log(T(1) - c)
            if defect != "no_probit_clamp":
                a, b = np.fmax(a, -mx), np.fmax(b, -mx)
            return -(y * a + (T(1) - y) * b)
        return T(0.5) * e * e - y * e


def np_hess(T, kind, y, w, g, eta, K=1, defect=None):
    with np.errstate(all="ignore"):
        guard = T(0) if defect == "no_w_guard" else (w <= 0).astype(T)
        if kind == POISSON:
            return w * y - g
        if kind == PROBIT:
            mx, c, pd = _fmax(T), np_cdf(T, eta), np_pdf(T, eta)
            c1 = T(1) - c
            a, b = T(1) / (c * c), T(1) / (c1 * c1)
            if defect != "no_probit_clamp":
                a, b = np.fmin(a, mx), np.fmin(b, mx)
            return w * (y * a + (T(1) - y) * b) * pd * pd + eta * g
        if kind == MULTINOMIAL:
            h = y * w / T(K) - g
            return h * (T(2) * (T(1) - T(K) * (h / (w + guard))))
        if kind == LOGIT:
            h = w * y - g
            return (h * (w - h)) / (w + guard)
        return w + T(0) * y


def _rows(x, nb, K, defect):
    """The (K, nb) view of a response-major array of nb K values; the 'row_major' defect reads [i K + k]."""
    return x.reshape(nb, K).T if defect == "row_major" else x.reshape(K, nb)


def np_multi_shifted(T, e, defect):
    """e (K, nb) -> e - max over the classes (the 'no_shift' defect subtracts nothing)."""
    return e if defect == "no_shift" else e - e.max(axis=0)[None, :]


def np_multi_grad(T, y, w, eta, nb, K, defect=None):
    """resid (nb K, response-major, laid out as the kernel lays it out under the defect)."""
    with np.errstate(all="ignore"):
        Y, E = _rows(y, nb, K, defect), _rows(eta, nb, K, defect)
        ex = np.exp(np_multi_shifted(T, E, defect))
        tot = np.zeros(nb, dtype=T)
        for k in range(K):
            tot = tot + ex[k]
        R = (Y - ex / tot[None, :]) * (w[:nb] / T(K))[None, :]
        out = np.empty(nb * K, dtype=T)
        _rows(out, nb, K, defect)[:] = R
        return out


def np_multi_loss_rows(T, Y, E, K, defect=None):
    """(-ye + log(se)) per row from (K, nb) arrays."""
    with np.errstate(all="ignore"):
        S = np_multi_shifted(T, E, defect)
        ye = np.zeros(S.shape[1], dtype=T)
        se = np.zeros(S.shape[1], dtype=T)
        for k in range(K):
            ye = ye + Y[k] * S[k]
            se = se + np.exp(S[k])
        return -ye + np.log(se)


def tree64(x):
    """Sum over axis 0 (64 lanes) in the order of the shuffle: lane 0 of x += shfl_down(x, off) for off = 32 .. 1."""
    while x.shape[0] > 1:
        h = x.shape[0] // 2
        x = x[:h] + x[h:]
    return x[0]


def reduce_model(T, terms, live):
    """The reduction of kernels_glm.hip over terms (k, n): thread g = i % 65536 adds its elements in order, the wave shuffle, the
    four waves of a workgroup in order, then the final reduce's shuffle and four waves over the 256 partials."""
    k, n = terms.shape
    trips = -(-n // STRIDE)
    pad = np.zeros((k, trips * STRIDE), dtype=T)
    pad[:, :n] = np.where(live[None, :], terms, T(0))
    x = pad.reshape(k, trips, RB, 4, 64)
    with np.errstate(all="ignore"):
        acc = np.zeros((k, RB, 4, 64), dtype=T)
        for t in range(trips):
            acc = acc + x[:, t]
        wave = tree64(np.moveaxis(acc, -1, 0))            # (k, RB, 4)
        part = np.zeros((k, RB), dtype=T)
        for w in range(4):
            part = part + wave[:, :, w]
        wv = tree64(np.moveaxis(part.reshape(k, 4, 64), -1, 0))   # (k, 4)
        s = np.zeros(k, dtype=T)
        for w in range(4):
            s = s + wv[:, w]
    return s


def _live(n, defect):
    i = np.arange(n)
    if defect == "drop_tail":
        return i < n - 1
    if defect == "skip_trip2":
        return i < STRIDE
    return np.ones(n, dtype=bool)


def _raise(T, h0, hmin, defect):
    le = (h0 < 0) if defect == "h0_lt" else (h0 <= 0)
    return np.where(h0 > 0, h0, T(0)) + hmin * le.astype(T)


def emulate_call(mode, dtype, a, defect=None):
    """The call in plain numpy in the value type, outputs written into `a` as the device call writes them; returns info."""
    T = NP_TYPE[dtype]
    if "sums" not in a:
        a["sums"] = prefill(dtype, 16)
    sums = np.full(16, T(SENTINEL), dtype=T)
    kind, n, K = int(a.get("kind", 0)), int(a.get("n", 0)), max(int(a.get("K", 1)), 1)
    nb = int(a.get("nb", 0))
    live = _live(n, defect)

    def put(name, val, mask=None):
        m = live if mask is None else mask
        a[name][m] = val[m]

    def red(*terms):
        sums[:len(terms)] = reduce_model(T, np.stack([t.astype(T) for t in terms]), live if terms[0].size == n else _live(terms[0].size, defect))

    with np.errstate(all="ignore"):
        if mode in (M_PREPARE, M_NULL):
            hmin = T(a["hmin"])
            cb, pre = kind == CALLBACK, kind in (CALLBACK, COX)
            h0 = a["hess"] if pre else np_hess(T, kind, a["y"], a["w"], a["resid"], a["eta"], K, defect)
            h = _raise(T, h0, hmin, defect)
            z = (a["irls_resid"] if mode == M_PREPARE else a["cb_z"]) if cb else a["resid"] / (h0 if defect == "raise_after_div" else h)
            iy = z + a["eta"] - a["off"]
            if mode == M_PREPARE:
                put("hess", h), put("irls_resid", z), put("irls_y", iy)
                red(h)
            else:
                red(h, h * iy)
        elif mode == M_WEIGHTS:
            wi = a["hess"] / T(a["hess_sum"])
            yi, ri = a["irls_y"], a["irls_resid"] + T(a["shift"])
            put("wts", wi), put("irls_resid", ri)
            t = (wi * yi, wi * yi * yi, wi * ri)
            red(*((t[0], t[2], t[1]) if defect == "swap_acc" else t))
        elif mode == M_FINISH:
            e = a["irls_y"] + a["off"] - a["irls_resid"] + T(a["shift"])
            put("eta", e)
            if kind == MULTINOMIAL:
                lv = _live(nb, defect)
                g = np_multi_grad(T, a["y"], a["w"], a["eta"], nb, K, defect)
                put("resid", g, np.tile(lv, K) if defect != "row_major" else np.repeat(lv, K))
            elif kind not in (CALLBACK, COX):
                put("resid", np_grad(T, kind, a["y"], a["w"], a["eta"], defect))
        elif mode == M_GRAD:
            if kind == MULTINOMIAL:
                lv = _live(nb, defect)
                g = np_multi_grad(T, a["y"], a["w"], a["eta"], nb, K, defect)
                put("resid", g, np.tile(lv, K) if defect != "row_major" else np.repeat(lv, K))
            else:
                put("resid", np_grad(T, kind, a["y"], a["w"], a["eta"], defect))
        elif mode == M_LOSS:
            if kind == MULTINOMIAL:
                l = np_multi_loss_rows(T, _rows(a["y"], nb, K, defect), _rows(a["eta"], nb, K, defect), K, defect)
                red(a["w"][:nb] * l / T(K))
            else:
                red(a["w"] * np_loss_term(T, kind, a["y"], a["eta"], defect))
        elif mode == M_LOSS2:
            e = a["eta"] + T(a["b0"]) + a["off"]
            l = np_loss_term(T, kind, a["y"], e, defect)
            red(a["w"] * l, a["wb"] * l)
        elif mode == M_MLOSS2:
            Y = _rows(a["y"], nb, K, defect)
            E = _rows(a["eta"], nb, K, defect) + a["b0v"][:K, None] + _rows(a["off"], nb, K, defect)
            if kind == MULTINOMIAL:
                l = np_multi_loss_rows(T, Y, E, K, defect) / T(K)
            else:
                acc = np.zeros(nb, dtype=T)
                for k in range(K):
                    acc = acc + (T(0.5) * E[k] * E[k] - Y[k] * E[k])
                l = acc / T(K)
            red(a["w"][:nb] * l, a["wb"][:nb] * l)
        elif mode == M_SET_ETA:
            put("eta", T(a["b0"]) + a["off"])
        elif mode == M_DOT:
            red((a["resid"] - a["resid_prev"]) * (a["eta"] - a["eta_prev"]))
        elif mode == M_REL:
            x, yv = a["wts"], a["prev"].copy()
            put("prev", x)
            d = np.abs(x - yv)
            r = np.where(yv > 0, d / yv, np.where(d > 0, T(1e30), T(0)))
            bad = np.isnan(r) | np.isnan(d)
            r = np.where(bad, T(0) if defect == "rel_nan_zero" else T(1e30), r)
            m = r[live].max() if live.any() else T(0)
            start = sums[15] if defect == "rel_no_reset" else T(0)
            sums[15] = max(start, m)
        elif mode == M_GATHER:
            cnt = int(a["cnt"])
            if cnt:
                a["dst"][:cnt] = a["src"][a["idx"][:cnt]]
        elif mode == M_SCATTER:
            cnt = int(a["cnt"])
            if cnt:
                a["dst"][a["idx"][:cnt]] = a["src"][:cnt]
    if mode in NSUMS or mode == M_REL:
        a["sums"][:] = sums
    return np.array([1, 0, 0, 0, 0, 0, 0, 0], dtype=np.int64)


# ---- the reference arithmetic: a value and a bound on the error of its value-type counterpart ------------------------------------
class Refused(AssertionError):
    """The input lies where the model cannot decide (a denominator, a log argument or a Hessian's sign within its own bound)."""


class Arith:
    def __init__(self, dtype):
        self.dtype, self.T = dtype, NP_TYPE[dtype]
        fi = np.finfo(self.T)
        self.u, self.fn = M(UNIT[dtype]), 2 * A_ULP * M(UNIT[dtype])
        self.mx, self.tiny = M(float(fi.max)), M(float(fi.smallest_subnormal))
        self.zero, self.one = (M(0), M(0)), (M(1), M(0))

    def ex(self, x):
        """A value-type number handed to the kernel: exact."""
        x = float(x)
        assert np.isfinite(x) and float(self.T(x)) == x
        return (M(x), M(0))

    def const(self, c):
        """A literal the kernel writes as T(c): rounded once."""
        c = M(c)
        return (c, self.u * abs(c))

    def rep(self, v):
        if abs(v) > self.mx:
            return False
        f = float(v)
        return M(f) == v and float(self.T(f)) == f

    def _rnd(self, v, p):
        if abs(v) + p > self.mx:
            raise Refused("the value type may overflow here: |%s| + %s" % (mpmath.nstr(v, 6), mpmath.nstr(p, 3)))
        if p == 0 and self.rep(v):
            return (v, p)
        return (v, p + self.u * (abs(v) + p) + self.tiny)

    def add(self, a, b):
        return self._rnd(a[0] + b[0], a[1] + b[1])

    def sub(self, a, b):
        return self._rnd(a[0] - b[0], a[1] + b[1])

    def neg(self, a):
        return (-a[0], a[1])

    def mul(self, a, b):
        return self._rnd(a[0] * b[0], abs(a[0]) * b[1] + abs(b[0]) * a[1] + a[1] * b[1])

    def div(self, a, b):
        if not abs(b[0]) > 2 * b[1]:
            raise Refused("a denominator within its own error bound of zero")
        v = a[0] / b[0]
        return self._rnd(v, (a[1] + abs(v) * b[1]) / (abs(b[0]) - b[1]))

    def _fn(self, v, p):
        if abs(v) + p > self.mx:
            raise Refused("the value type may overflow in a function call")
        return (v, p + self.fn * (abs(v) + p) + (1 + 2 * A_ULP) * self.tiny)

    def exp(self, a):
        v = ctx.exp(a[0])
        return self._fn(v, v * ctx.expm1(a[1]))

    def log(self, a):
        if not a[0] > 2 * a[1]:
            raise Refused("a log argument within its own error bound of zero")
        return self._fn(ctx.log(a[0]), -ctx.log1p(-a[1] / a[0]))

    def erf(self, a):
        lo = max(abs(a[0]) - a[1], M(0))
        return self._fn(ctx.erf(a[0]), 2 / ctx.sqrt(ctx.pi) * ctx.exp(-lo * lo) * a[1])

    def vmax(self, xs):
        return (max(x[0] for x in xs), max(x[1] for x in xs))

    # ---- the family members, operation for operation as kernels_glm.hip writes them ----
    def cdf(self, x):
        if abs(x[0]) >= PROBIT_SAT[self.dtype] and x[1] == 0:     # erf has saturated: c is exactly 0 or 1
            return self.zero if x[0] < 0 else self.one
        return self.mul(self.ex(0.5), self.add(self.one, self.erf(self.mul(x, self.const(ctx.sqrt(M(0.5)))))))

    def pdf(self, x):
        return self.mul(self.const(1 / ctx.sqrt(2 * ctx.pi)), self.exp(self.mul(self.mul(self.ex(-0.5), x), x)))

    def recip_clamped(self, c):
        """min(1 / c, max)"""
        if c == self.zero:
            return (self.mx, M(0))
        r = self.div(self.one, c)
        if r[0] + r[1] >= self.mx:
            raise Refused("1 / c at the clamp")
        return r

    def log_clamped(self, c):
        """max(log c, -max)"""
        if c == self.zero:
            return (-self.mx, M(0))
        if c == self.one:
            return self.zero
        return self.log(c)

    def guard(self, w):
        """w + T(w <= 0)"""
        return self.add(w, self.one if w[0] <= 0 else self.zero)

    def grad(self, kind, y, w, eta):
        if kind == LOGIT:
            return self.mul(w, self.sub(y, self.div(self.one, self.add(self.one, self.exp(self.neg(eta))))))
        if kind == POISSON:
            return self.mul(w, self.sub(y, self.exp(eta)))
        if kind == PROBIT:
            c = self.cdf(eta)
            t = self.sub(self.mul(y, self.recip_clamped(c)), self.mul(self.sub(self.one, y), self.recip_clamped(self.sub(self.one, c))))
            return self.mul(self.mul(w, self.pdf(eta)), t)
        return self.mul(w, self.sub(y, eta))

    def loss_term(self, kind, y, e):
        if kind == LOGIT:
            if e[1] != 0 and abs(e[0]) <= 2 * e[1]:
                raise Refused("the sign of eta within its own error bound")
            ind = self.one if e[0] > 0 else self.zero
            ab = (abs(e[0]), e[1])
            return self.add(self.mul(self.sub(ind, y), e), self.log(self.add(self.one, self.exp(self.neg(ab)))))
        if kind == POISSON:
            return self.add(self.mul(self.neg(e), y), self.exp(e))
        if kind == PROBIT:
            c = self.cdf(e)
            return self.neg(self.add(self.mul(y, self.log_clamped(c)), self.mul(self.sub(self.one, y), self.log_clamped(self.sub(self.one, c)))))
        return self.sub(self.mul(self.mul(self.ex(0.5), e), e), self.mul(y, e))

    def hess(self, kind, y, w, g, eta, K=1):
        if kind == POISSON:
            return self.sub(self.mul(w, y), g)
        if kind == PROBIT:
            c, pd = self.cdf(eta), self.pdf(eta)
            c1 = self.sub(self.one, c)
            t = self.add(self.mul(y, self.recip_clamped(self.mul(c, c))), self.mul(self.sub(self.one, y), self.recip_clamped(self.mul(c1, c1))))
            return self.add(self.mul(self.mul(self.mul(w, t), pd), pd), self.mul(eta, g))
        if kind == MULTINOMIAL:
            Km = self.ex(K)
            h = self.sub(self.div(self.mul(y, w), Km), g)
            return self.mul(h, self.mul(self.ex(2), self.sub(self.one, self.mul(Km, self.div(h, self.guard(w))))))
        if kind == LOGIT:
            h = self.sub(self.mul(w, y), g)
            return self.div(self.mul(h, self.sub(w, h)), self.guard(w))
        return w

    def raised(self, h0, hmin):
        """(h0 > 0 ? h0 : 0) + hmin * T(h0 <= 0); returns (h, whether the raise fired)."""
        if (h0[0] == 0 and h0[1] == 0) or h0[0] + h0[1] < 0:
            return hmin, True
        if h0[0] - h0[1] > 0:
            return h0, False
        raise Refused("the sign of a Hessian within its own error bound: %s +- %s" % (mpmath.nstr(h0[0], 6), mpmath.nstr(h0[1], 3)))

    def multi_shift(self, es):
        mx = self.vmax(es)
        return [self.sub(e, mx) if not (e[1] == 0 and mx[1] == 0 and e[0] == mx[0]) else self.zero for e in es]

    def multi_grad_row(self, ys, w, etas, K):
        sh = self.multi_shift(etas)
        ex = [self.exp(s) for s in sh]
        tot = self.zero
        for x in ex:
            tot = self.add(tot, x)
        wk = self.div(w, self.ex(K))
        return [self.mul(self.sub(y, self.div(x, tot)), wk) for y, x in zip(ys, ex)]

    def multi_loss_row(self, ys, es):
        """-ye + log(se) of one row"""
        sh = self.multi_shift(es)
        ye, se = self.zero, self.zero
        for y, s in zip(ys, sh):
            ye = self.add(ye, self.mul(y, s))
            se = self.add(se, self.exp(s))
        return self.add(self.neg(ye), self.log(se))


def ratio_of(dev, ref, what=""):
    """max |dev - v| / e over a list of references (v, e); where e = 0 the value must be exact.  Never NaN, never infinite."""
    dev = np.asarray(dev).reshape(-1)
    assert dev.size == len(ref), (dev.size, len(ref))
    assert np.isfinite(dev).all(), "%s: a non-finite output at %s" % (what, np.flatnonzero(~np.isfinite(dev))[:4].tolist())
    worst = 0.0
    for q, (x, (v, e)) in enumerate(zip(dev, ref)):
        err = abs(M(float(x)) - v)
        if e == 0:
            assert err == 0, "%s[%d]: %r differs from the exact %s" % (what, q, x, mpmath.nstr(v, 20))
        else:
            worst = max(worst, float(err / e))
    return worst


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def _fractions(rng, T, shape, choices):
    return rng.choice(np.array(choices, dtype=T), size=shape).astype(T)


@functools.lru_cache(maxsize=None)
def base_arrays(kind, dtype, K=1):
    """Everything a call on the rounding leg may need, as (K, NB) arrays (one row per class; K = 1 for the scalar kinds): y, w, wb,
    eta, off, resid (the model's gradient at eta), and the arrays of the launchers that take no kind."""
    T = NP_TYPE[dtype]
    rng = _rng("glm base %s %s K%d" % (KIND_NAME[kind], dtype, K))
    multi = kind == MULTINOMIAL
    NB = NBASE_MULTI if multi else NBASE
    R = RANGES[(GAUSSIAN if kind in (GAUSSIAN_IRLS, CALLBACK, COX) else kind, dtype)]
    eta = rng.uniform(-R, R, size=(K, NB)).astype(T)
    eta[0, :5] = [0.0, 2.0 ** -10, -2.0 ** -10, R, -R]
    if multi and K > 1:
        eta[:, 5] = eta[0, 5]                                    # a row whose classes are all equal
    w_row = _fractions(rng, T, NB, (0.25, 0.5, 1.0, 1.5, 2.0)) * (1 + rng.randint(0, 8, size=NB) / T(8))
    w = np.tile(w_row.astype(T), (K, 1))
    if multi:
        y = np.zeros((K, NB), dtype=T)
        y[rng.randint(0, K, size=NB), np.arange(NB)] = 1
    elif kind == POISSON:
        y = rng.randint(0, 6, size=(K, NB)).astype(T)
    elif kind in (LOGIT, PROBIT):
        y = _fractions(rng, T, (K, NB), (0.0, 1.0, 0.0, 1.0, 0.25, 0.625))
    else:
        y = rng.normal(size=(K, NB)).astype(T)
    out = dict(eta=eta, w=w, y=y)
    out["wb"] = (w * _fractions(rng, T, (1, NB), (0.0, 0.5, 1.0, 1.25))).astype(T)
    out["off"] = (rng.normal(size=(K, NB)) * 0.25).astype(T)
    if multi:
        out["resid"] = np_multi_grad(T, y.reshape(-1), w.reshape(-1), eta.reshape(-1), NB, K).reshape(K, NB)
    else:
        out["resid"] = np_grad(T, kind, y, w, eta)
    for name in ("irls_resid", "cb_z", "resid_prev", "eta_prev"):
        out[name] = rng.normal(size=(K, NB)).astype(T)
    # FINISH forms irls_y + off - irls_resid + shift: back at eta up to rounding, so that it stays inside the range
    out["irls_y"] = (eta + out["irls_resid"] - out["off"] - T(SCALARS["shift"])).astype(T)
    out["hess"] = rng.uniform(0.05, 2.0, size=(K, NB)).astype(T)
    for v in out.values():
        v.setflags(write=False)
    return out


SCALARS = dict(hmin=HMIN, hess_sum=37.5, shift=-0.375, b0=0.3125)     # (all representable in float32 but hmin, which is T(1e-24))
B0V = (0.25, -0.5, 0.125, 0.75, -0.375, 0.5, -0.125)
INPUTS = {M_PREPARE: ("y", "w", "eta", "resid", "off"), M_WEIGHTS: ("hess", "irls_y", "irls_resid"),
          M_FINISH: ("y", "w", "irls_y", "off", "irls_resid"), M_NULL: ("y", "w", "eta", "resid", "off"),
          M_GRAD: ("y", "w", "eta"), M_LOSS: ("y", "w", "eta"), M_LOSS2: ("y", "w", "wb", "eta", "off"),
          M_MLOSS2: ("y", "w", "wb", "eta", "off"), M_SET_ETA: ("off",), M_DOT: ("resid", "resid_prev", "eta", "eta_prev")}


def tiled(x, n):
    """(K, NB) -> the response-major array of n = nb K values whose row i is base row i % NB."""
    K, NB = x.shape
    return np.ascontiguousarray(x[:, np.arange(n // K) % NB]).reshape(-1)


def call_inputs(mode, kind, dtype, n, K, base):
    """The arrays of one call from (K, NB) base arrays; outputs pre-filled."""
    a = dict(kind=kind, n=n, K=K, nb=n // K)
    a.update(SCALARS)
    pre = kind in (CALLBACK, COX)
    for name in INPUTS[mode]:
        if name in ("w", "wb") and mode == M_MLOSS2:
            a[name] = tiled(base[name][:1], n // K)
        else:
            a[name] = tiled(base[name], n)
    if mode == M_MLOSS2:
        a["b0v"] = np.array(B0V[:K], dtype=NP_TYPE[dtype])
    if mode in (M_PREPARE, M_NULL) and pre:
        a["hess"] = tiled(base["hess"], n)
        if kind == CALLBACK:
            a["irls_resid" if mode == M_PREPARE else "cb_z"] = tiled(base["cb_z"], n)
    for name in OUTPUTS[mode]:
        if name not in a:
            a[name] = prefill(dtype, n)
    return a


# ---- references of one call on its base arrays -------------------------------------------------------------------------------------
def reference(mode, kind, dtype, K, base, scal=SCALARS, own=None):
    """Arith references on (K, NB) base arrays: {'elem': {output: [(v, e)] * (K NB), response-major}, 'terms': [[(v, e)] per
    element or row] per accumulator, 'raised': flags of PREPARE / NULL_STEP}.  `own`: the device's own eta output (K, NB), which
    FINISH's gradient is judged from."""
    ar = Arith(dtype)
    T = NP_TYPE[dtype]
    Kc, NB = next(iter(base.values())).shape
    ex = lambda name: [[ar.ex(v) for v in row] for row in base[name]]     # noqa: E731
    flat = lambda rows: [x for row in rows for x in row]                    # noqa: E731
    sc = {k: ar.ex(T(v)) for k, v in scal.items() if k != "b0v"}
    b0v = scal.get("b0v", B0V)
    out = dict(elem={}, terms=[], raised=None)
    if mode in (M_PREPARE, M_NULL):
        cb, pre = kind == CALLBACK, kind in (CALLBACK, COX)
        eta, off = ex("eta"), ex("off")
        H, Z, IY, RS = [], [], [], []
        for k in range(Kc):
            for i in range(NB):
                if pre:
                    h0 = ar.ex(base["hess"][k, i])
                else:
                    h0 = ar.hess(kind, ar.ex(base["y"][k, i]), ar.ex(base["w"][k, i]), ar.ex(base["resid"][k, i]), eta[k][i], K)
                h, fired = ar.raised(h0, sc["hmin"])
                z = ar.ex(base["cb_z"][k, i]) if cb else ar.div(ar.ex(base["resid"][k, i]), h)
                H.append(h), Z.append(z), RS.append(fired)
                IY.append(ar.sub(ar.add(z, eta[k][i]), off[k][i]))
        out["raised"] = np.array(RS)
        if mode == M_PREPARE:
            out["elem"] = dict(hess=H, irls_resid=Z, irls_y=IY)
            out["terms"] = [H]
        else:
            out["terms"] = [H, [ar.mul(h, iy) for h, iy in zip(H, IY)]]
    elif mode == M_WEIGHTS:
        W, RI, t0, t1, t2 = [], [], [], [], []
        for h, yi, r in zip(flat(ex("hess")), flat(ex("irls_y")), flat(ex("irls_resid"))):
            wi, ri = ar.div(h, sc["hess_sum"]), ar.add(r, sc["shift"])
            wy = ar.mul(wi, yi)
            W.append(wi), RI.append(ri), t0.append(wy), t1.append(ar.mul(wy, yi)), t2.append(ar.mul(wi, ri))
        out["elem"], out["terms"] = dict(wts=W, irls_resid=RI), [t0, t1, t2]
    elif mode == M_FINISH:
        E = [ar.add(ar.sub(ar.add(iy, o), r), sc["shift"]) for iy, o, r in zip(flat(ex("irls_y")), flat(ex("off")), flat(ex("irls_resid")))]
        out["elem"]["eta"] = E
        if own is not None and kind not in (CALLBACK, COX):
            b2 = dict(base)
            b2["eta"] = own
            out["elem"]["resid"] = reference(M_GRAD, kind, dtype, K, b2)["elem"]["resid"]
    elif mode == M_GRAD:
        if kind == MULTINOMIAL:
            R = [[None] * NB for _ in range(K)]
            for i in range(NB):
                g = ar.multi_grad_row([ar.ex(base["y"][k, i]) for k in range(K)], ar.ex(base["w"][0, i]), [ar.ex(base["eta"][k, i]) for k in range(K)], K)
                for k in range(K):
                    R[k][i] = g[k]
            out["elem"]["resid"] = flat(R)
        else:
            out["elem"]["resid"] = [ar.grad(kind, y, w, e) for y, w, e in zip(flat(ex("y")), flat(ex("w")), flat(ex("eta")))]
    elif mode == M_LOSS:
        if kind == MULTINOMIAL:
            Km = ar.ex(K)
            out["terms"] = [[ar.div(ar.mul(ar.ex(base["w"][0, i]), ar.multi_loss_row([ar.ex(base["y"][k, i]) for k in range(K)],
                                                                                     [ar.ex(base["eta"][k, i]) for k in range(K)])), Km)
                             for i in range(NB)]]
        else:
            out["terms"] = [[ar.mul(w, ar.loss_term(kind, y, e)) for y, w, e in zip(flat(ex("y")), flat(ex("w")), flat(ex("eta")))]]
    elif mode == M_LOSS2:
        ta, tb = [], []
        for y, wa, wb, b, o in zip(*(flat(ex(k)) for k in ("y", "w", "wb", "eta", "off"))):
            l = ar.loss_term(kind, y, ar.add(ar.add(b, sc["b0"]), o))
            ta.append(ar.mul(wa, l)), tb.append(ar.mul(wb, l))
        out["terms"] = [ta, tb]
    elif mode == M_MLOSS2:
        Km = ar.ex(K)
        ta, tb = [], []
        for i in range(NB):
            ys = [ar.ex(base["y"][k, i]) for k in range(K)]
            es = [ar.add(ar.add(ar.ex(base["eta"][k, i]), ar.ex(T(b0v[k]))), ar.ex(base["off"][k, i])) for k in range(K)]
            if kind == MULTINOMIAL:
                l = ar.div(ar.multi_loss_row(ys, es), Km)
            else:
                acc = ar.zero
                for y, e in zip(ys, es):
                    acc = ar.add(acc, ar.loss_term(GAUSSIAN, y, e))
                l = ar.div(acc, Km)
            ta.append(ar.mul(ar.ex(base["w"][0, i]), l)), tb.append(ar.mul(ar.ex(base["wb"][0, i]), l))
        out["terms"] = [ta, tb]
    elif mode == M_SET_ETA:
        out["elem"]["eta"] = [ar.add(sc["b0"], o) for o in flat(ex("off"))]
    elif mode == M_DOT:
        out["terms"] = [[ar.mul(ar.sub(a_, a0), ar.sub(b_, b0)) for a_, a0, b_, b0 in
                         zip(*(flat(ex(k)) for k in ("resid", "resid_prev", "eta", "eta_prev")))]]
    return out


@functools.lru_cache(maxsize=None)
def base_reference(mode, kind, dtype, K):
    return reference(mode, kind, dtype, K, base_arrays(kind, dtype, K))


def reduction_depth(n_terms):
    """Roundings on the longest path of a sum: the thread's chain, 6 shuffle steps, 4 waves, and the final reduce's 6 + 4."""
    return -(-n_terms // STRIDE) + 6 + 4 + 6 + 4


def sum_check(dev, terms, counts, n_terms, dtype, what=""):
    """|dev - sum_j counts_j t_j| against (1 + gamma_m) sum counts_j e_j + gamma_m sum counts_j |t_j|; returns the ratio."""
    g = M(gamma(reduction_depth(n_terms), UNIT[dtype]))
    S = sum(int(c) * t[0] for c, t in zip(counts, terms))
    bound = (1 + g) * sum(int(c) * t[1] for c, t in zip(counts, terms)) + g * sum(int(c) * abs(t[0]) for c, t in zip(counts, terms))
    assert np.isfinite(dev), "%s: a non-finite sum" % what
    err = abs(M(float(dev)) - S)
    if bound == 0:
        assert err == 0, "%s: %r differs from the exact %s" % (what, dev, mpmath.nstr(S, 20))
        return 0.0
    return float(err / bound)


def same_bits(x, y):
    return np.array_equal(bits(np.ascontiguousarray(x)), bits(np.ascontiguousarray(y)))


def twice(call, mode, dtype, a):
    """Runs the call twice on copies of `a`; a reduction must repeat its bits.  Returns the first run's arrays."""
    a1, a2 = copy_inputs(a), copy_inputs(a)
    call(mode, dtype, a1)
    if mode in NSUMS or mode == M_REL:
        call(mode, dtype, a2)
        assert same_bits(a1["sums"], a2["sums"]), "%s: the reduction did not repeat its bits" % MODE_NAME[mode]
    return a1


def check_sums_footprint(mode, dtype, sums):
    """Result slots hold numbers, every other of the 16 slots still holds the sentinel."""
    T = NP_TYPE[dtype]
    used = list(range(NSUMS.get(mode, 0))) + ([15] if mode == M_REL else [])
    for q in range(16):
        if q not in used:
            assert sums[q] == T(SENTINEL), "%s wrote sums[%d]" % (MODE_NAME[mode], q)
        else:
            assert not (sums[q] == T(SENTINEL)), "%s left sums[%d] unwritten" % (MODE_NAME[mode], q)


# ---- the rounding leg ---------------------------------------------------------------------------------------------------------------
def shapes_of(mode, kind):
    if kind == MULTINOMIAL and mode == M_NULL:
        return tuple((n, 3) for n in N_LIST)
    if mode == M_MLOSS2 or (kind == MULTINOMIAL and mode != M_NULL):
        return MULTI_SHAPES
    return tuple((n, 1) for n in N_LIST)


def run_rounding(call, mode, kind, dtype, shapes=None):
    """The base call against Arith, then every shape against the base call's bits and the tiled sums.  `call(mode, dtype, a)` runs
    one call in place.  Returns {figure: worst error / bound}."""
    ratios = {}

    def note(key, r):
        ratios[key] = max(ratios.get(key, 0.0), r)

    shapes = shapes_of(mode, kind) if shapes is None else shapes
    # NULL_STEP with the multinomial member is elementwise over one class, K a parameter (the solver calls it class by class)
    null_multi = kind == MULTINOMIAL and mode == M_NULL
    row_coupled = mode == M_MLOSS2 or (kind == MULTINOMIAL and not null_multi)
    for K in sorted({k for _, k in shapes}):
        Kb = K if row_coupled else 1
        base = base_arrays(kind, dtype, K if (row_coupled or null_multi) else 1)
        if null_multi:
            base = {k: v[:1] for k, v in base.items()}
        NB = base["y"].shape[1]
        a0 = call_inputs(mode, kind, dtype, NB * Kb, Kb, base)
        a0["K"] = K
        b = twice(call, mode, dtype, a0)
        if mode == M_FINISH:
            ref = reference(mode, kind, dtype, K, base, own=b["eta"].reshape(Kb, NB))
        elif null_multi:
            ref = reference(mode, kind, dtype, K, base)
        else:
            ref = base_reference(mode, kind, dtype, K)
        for name, r in ref["elem"].items():
            note(name, ratio_of(b[name], r, "%s %s" % (MODE_NAME[mode], name)))
        for name in OUTPUTS[mode]:
            if name not in ref["elem"]:                           # (FINISH under CALLBACK / COX: resid stays as it was)
                assert same_bits(b[name], a0[name]), "%s changed %s" % (MODE_NAME[mode], name)
        if ref["raised"] is not None and mode == M_PREPARE:
            raise_bits_check(dtype, a0, b, ref["raised"], kind)
        for nK, K2 in shapes:
            if K2 != K:
                continue
            n = nK * Kb
            a = call_inputs(mode, kind, dtype, n, Kb, base)
            a["K"] = K
            d = twice(call, mode, dtype, a)
            for name in OUTPUTS[mode]:
                want = tiled(b[name].reshape(Kb, NB), n)
                assert same_bits(d[name], want), "%s n=%d K=%d: %s differs from the base call's bits at %s" % (
                    MODE_NAME[mode], n, K, name, np.flatnonzero(bits(d[name]) != bits(want))[:4].tolist())
            for k in INPUTS[mode]:
                if k not in OUTPUTS[mode]:
                    assert same_bits(d[k], a[k])
            if mode in NSUMS:
                check_sums_footprint(mode, dtype, d["sums"])
                if row_coupled and mode in (M_LOSS, M_MLOSS2):    # one term per row
                    rows = n // Kb
                    counts = np.bincount(np.arange(rows) % NB, minlength=NB)
                else:                                             # one term per element, response-major
                    rows = n
                    counts = np.tile(np.bincount(np.arange(n // Kb) % NB, minlength=NB), Kb)
                for q, terms in enumerate(ref["terms"]):
                    note("sum%d" % q, sum_check(d["sums"][q], terms, counts, rows, dtype, "%s n=%d K=%d sums[%d]" % (MODE_NAME[mode], n, K, q)))
    return ratios


def raise_bits_check(dtype, a_in, a_out, fired, kind):
    """Where the raise fired: hess == hmin, z == resid / hmin and irls_y == z + eta - off, bit for bit in numpy's value type."""
    T = NP_TYPE[dtype]
    f = np.asarray(fired)
    if not f.any():
        return
    hmin = T(a_in["hmin"])
    assert (a_out["hess"][f] == hmin).all(), "a raised Hessian is not hessian_min"
    with np.errstate(all="ignore"):
        if kind != CALLBACK:
            assert same_bits(a_out["irls_resid"][f], (a_in["resid"][f] / hmin).astype(T)), "z is not resid / hessian_min where the raise fired"
        assert same_bits(a_out["irls_y"][f], (a_out["irls_resid"][f] + a_in["eta"][f] - a_in["off"][f]).astype(T)), "irls_y is not z + eta - off"


# ---- the decision leg ---------------------------------------------------------------------------------------------------------------
def decision_arrays(kind, dtype, K=1):
    """(K, nd) arrays where a branch decides (see the module docstring), in the layout of base_arrays."""
    T = NP_TYPE[dtype]
    if kind == MULTINOMIAL:
        S = SHIFT_ETA[dtype]
        cols = []
        pats = [[S] * K, [-S] * K, [S if k == 0 else -S for k in range(K)], [-S if k == 0 else S for k in range(K)],
                [S - k for k in range(K)], [0.0] * K, [-S + 3 * k for k in range(K)],
                # past exp's overflow threshold (709.8 / 88.7): without the shift these are inf / inf
                [S + 10] * K, [S + 4 * (k + 3) for k in range(K)], [-S - 10 if k else S + 10 for k in range(K)]]
        for wv in (1.0, 0.0):                                    # (w = 0: the `w <= 0` guard of the Hessian)
            for hot in (0, K - 1):
                for p in pats:
                    cols.append((p, wv, hot))
        nd = len(cols)
        eta = np.array([c[0] for c in cols], dtype=T).T.copy()
        w = np.tile(np.array([c[1] for c in cols], dtype=T), (K, 1))
        y = np.zeros((K, nd), dtype=T)
        y[[c[2] for c in cols], np.arange(nd)] = 1
        resid = np_multi_grad(T, y.reshape(-1), w.reshape(-1), eta.reshape(-1), nd, K).reshape(K, nd)
    else:
        rows = []   # (y, w, eta, resid or None: the model's gradient)
        if kind == LOGIT:
            for yv in (0.0, 1.0, 0.25):
                rows += [(yv, 0.0, 1.5, None), (yv, 0.0, -3.0, None),              # w = 0: guard and raise
                         (yv, 0.5, 2.0, 0.5 * yv), (yv, 2.0, -1.0, 2.0 * yv),      # resid == w y exactly: h = 0, the Hessian is exactly 0
                         (yv, 0.5, 2.0, 0.5 * yv - 0.5)]                          # resid == w (y - 1): h = w, w - h = 0
        elif kind == POISSON:
            for yv in (0.0, 1.0, 3.0):
                rows += [(yv, 0.0, 0.5, None), (yv, 1.5, -2.0, 1.5 * yv), (yv, 0.5, 1.0, 0.5 * yv)]   # the gradient of an underflowed exp(eta)
        elif kind == PROBIT:
            P = PROBIT_SAT[dtype]
            for yv in (0.0, 1.0, 0.25):
                for wv in (1.0, 0.5, 0.0):
                    rows += [(yv, wv, P, None), (yv, wv, -P, None), (yv, wv, P + 1.5, None), (yv, wv, -P - 0.25, None)]
        elif kind in (GAUSSIAN, GAUSSIAN_IRLS):
            rows += [(1.0, 0.0, 0.5, None), (-2.0, 0.0, -1.0, None), (0.5, 1.0, 0.25, None)]
        y = np.array([[r[0] for r in rows]], dtype=T)
        w = np.array([[r[1] for r in rows]], dtype=T)
        eta = np.array([[r[2] for r in rows]], dtype=T)
        resid = np_grad(T, kind, y, w, eta)
        for q, r in enumerate(rows):
            if r[3] is not None:
                resid[0, q] = r[3]
        nd = len(rows)
    rng = _rng("glm decision %s %s K%d" % (KIND_NAME[kind], dtype, K))
    out = dict(y=y, w=w, eta=eta, resid=resid.astype(T), wb=(w * T(0.5)).astype(T))
    out["off"] = (rng.randint(-4, 5, size=y.shape) / 8.0).astype(T)
    return out


def run_decision(call, mode, kind, dtype, K=1):
    """One decision array through one launcher: elementwise modes in one call, reductions element by element (n = 1, or one row),
    so that every term is seen on its own.  Returns the ratios."""
    T = NP_TYPE[dtype]
    ratios = {}
    row_coupled = mode == M_MLOSS2 or (kind == MULTINOMIAL and mode != M_NULL)
    base = decision_arrays(kind, dtype, K)
    if kind == MULTINOMIAL and K > 1 and mode in (M_PREPARE, M_NULL):
        # (with w > 0 a saturated row's Hessian is zero only up to rounding: Arith refuses it; the w = 0 rows decide exactly)
        keep = base["w"][0] == 0
        base = {k: np.ascontiguousarray(v[:, keep]) for k, v in base.items()}
    if kind == MULTINOMIAL and mode == M_NULL:
        base = {k: v[:1] for k, v in base.items()}
    if mode in (M_PREPARE, M_NULL):
        # (float32, probit: a clamped gradient of 1e24 over hessian_min = 1e-24 overflows in the formula itself: not a case)
        with np.errstate(all="ignore"):
            keep = np.isfinite(base["resid"] / T(HMIN)).all(axis=0)
        base = {k: np.ascontiguousarray(v[:, keep]) for k, v in base.items()}
    Kb = K if row_coupled else 1
    nd = base["y"].shape[1]
    scal = dict(SCALARS, b0=0.0, b0v=(0.0,) * 7) if mode in (M_LOSS2, M_MLOSS2) else SCALARS
    if mode in (M_LOSS2, M_MLOSS2):                               # eta + b0 + off must stay exactly eta where eta decides
        base = dict(base, off=np.zeros_like(base["off"]))
    if mode in OUTPUTS and OUTPUTS[mode]:
        a0 = call_inputs(mode, kind, dtype, nd * Kb, Kb, base)
        a0.update({k: v for k, v in scal.items() if k != "b0v"})
        a0["K"] = K
        b = twice(call, mode, dtype, a0)
        ref = reference(mode, kind, dtype, K, base, scal, own=b["eta"].reshape(Kb, nd) if mode == M_FINISH else None)
        for name, r in ref["elem"].items():
            ratios[name] = ratio_of(b[name], r, "decision %s %s %s" % (MODE_NAME[mode], KIND_NAME[kind], name))
        if mode == M_PREPARE:
            raise_bits_check(dtype, a0, b, ref["raised"], kind)
            ratios["raised"] = int(ref["raised"].sum())
    if mode in NSUMS:
        ref = reference(mode, kind, dtype, K, base, scal)
        for i in range(nd):
            one = {k: v[:, i:i + 1] for k, v in base.items()}
            a = call_inputs(mode, kind, dtype, Kb, Kb, one)
            a.update({k: v for k, v in scal.items() if k != "b0v"})
            a["K"] = K
            if mode == M_MLOSS2:
                a["b0v"] = np.zeros(K, dtype=T)
            d = twice(call, mode, dtype, a)
            check_sums_footprint(mode, dtype, d["sums"])
            for q, terms in enumerate(ref["terms"]):
                what = "decision %s %s element %d sums[%d]" % (MODE_NAME[mode], KIND_NAME[kind], i, q)
                if len(terms) == nd:                              # the one term of the call: nothing but zeros is added to it
                    r = ratio_of(d["sums"][q:q + 1], [terms[i]], what)
                else:                                             # (PREPARE on a multinomial row: its K elements)
                    r = sum_check(d["sums"][q], [terms[k * nd + i] for k in range(Kb)], np.ones(Kb, dtype=int), Kb, dtype, what)
                ratios["sum%d" % q] = max(ratios.get("sum%d" % q, 0.0), r)
    return ratios


def run_prefilled_kinds(call, dtype, modes=(M_PREPARE, M_NULL, M_FINISH)):
    """CALLBACK and COX: PREPARE and NULL_STEP read hess (zero and negative entries are raised), z comes from irls_resid / cb_z only
    for CALLBACK; FINISH leaves resid as it was.  y, w (and resid for CALLBACK) are not handed in at all."""
    T = NP_TYPE[dtype]
    ratios = {}
    for kind in (CALLBACK, COX):
        base = dict(base_arrays(kind, dtype, 1))
        h = base["hess"].copy()
        h[0, :6] = [0.0, -0.0, -1.5, 2.0 ** -40, -2.0 ** -40, 3.0]
        base["hess"] = h
        for mode in modes:
            a0 = call_inputs(mode, kind, dtype, NBASE, 1, base)
            for k in ("y", "w") + (("resid",) if kind == CALLBACK and mode != M_FINISH else ()):
                a0[k] = None
            b = twice(call, mode, dtype, a0)
            ref = reference(mode, kind, dtype, 1, base)
            for name, r in ref["elem"].items():
                ratios["%s %s" % (KIND_NAME[kind], name)] = ratio_of(b[name], r, "%s %s %s" % (KIND_NAME[kind], MODE_NAME[mode], name))
            if mode == M_PREPARE:
                assert ref["raised"][:6].tolist() == [True, True, True, False, True, False]
                raise_bits_check(dtype, a0, b, ref["raised"], kind)
                if kind == CALLBACK:
                    assert same_bits(b["irls_resid"], a0["irls_resid"]), "CALLBACK: z must be the irls_resid handed in"
            if mode == M_FINISH:
                assert is_prefill(b["resid"]).all(), "%s: FINISH wrote resid" % KIND_NAME[kind]
            if mode in NSUMS:
                check_sums_footprint(mode, dtype, b["sums"])
                for q, terms in enumerate(ref["terms"]):
                    ratios["%s sum%d" % (KIND_NAME[kind], q)] = sum_check(b["sums"][q], terms, np.ones(NBASE, dtype=int), NBASE, dtype)
    return ratios


def run_overflow_decisions(call, dtype):
    """Where the value type overflows on the way and the expected value is written out in numpy (see the module docstring)."""
    T = NP_TYPE[dtype]
    mx = _fmax(T)
    # logit: exp(-eta) overflows at eta = -L, underflows at +L: the gradient saturates to w y and w (y - 1)
    L = T(LOGIT_SAT[dtype])
    y = np.array([0, 1, 0.25, 0, 1, 0.25], dtype=T)
    w = np.array([0.5, 1.5, 2, 0.5, 1.5, 2], dtype=T)
    eta = np.array([-L, -L, -L, L, L, L], dtype=T)
    a = dict(kind=LOGIT, n=6, K=1, nb=6, y=y, w=w, eta=eta, resid=prefill(dtype, 6))
    call(M_GRAD, dtype, a)
    want = np.concatenate([w[:3] * y[:3], w[3:] * (y[3:] - T(1))]).astype(T)
    assert same_bits(a["resid"], want), "the logit gradient does not saturate to w y / w (y - 1): %r" % a["resid"]
    # ... and its loss there is (T(e > 0) - y) e + log(1 + 0)
    for q in range(6):
        b = dict(kind=LOGIT, n=1, K=1, nb=1, y=y[q:q + 1].copy(), w=w[q:q + 1].copy(), eta=eta[q:q + 1].copy())
        call(M_LOSS, dtype, b)
        want1 = w[q] * ((T(eta[q] > 0) - y[q]) * eta[q])
        assert b["sums"][0] == want1, "logit loss at eta = %r: %r, expected %r" % (eta[q], b["sums"][0], want1)
    # Poisson loss: min(-eta, max) y + exp(eta) at eta = -inf and hugely negative eta
    for e in (T(-np.inf), T(POISSON_HUGE[dtype])):
        for yv in (T(0), T(1), T(0.5)):
            for mode in (M_LOSS, M_LOSS2):
                b = dict(kind=POISSON, n=1, K=1, nb=1, y=np.array([yv], dtype=T), w=np.array([1], dtype=T), eta=np.array([e], dtype=T))
                if mode == M_LOSS2:
                    b.update(wb=np.array([0.5], dtype=T), off=np.zeros(1, dtype=T), b0=0.0)
                call(mode, dtype, b)
                with np.errstate(all="ignore"):
                    want1 = np.fmin(-e, mx) * yv + np.exp(e)
                assert np.isfinite(want1) and not np.isnan(b["sums"][0])
                assert b["sums"][0] == want1, "Poisson loss at eta = %r, y = %r: %r, expected %r" % (e, yv, b["sums"][0], want1)
                if mode == M_LOSS2:
                    assert b["sums"][1] == T(0.5) * want1
    # Poisson gradient where exp(eta) has underflowed to zero: exactly w y, so that the Hessian w y - resid is exactly 0
    e = np.full(3, EXP_ZERO[dtype], dtype=T)
    y3, w3 = np.array([0, 1, 3], dtype=T), np.array([1.5, 0.5, 2], dtype=T)
    a = dict(kind=POISSON, n=3, K=1, nb=3, y=y3, w=w3, eta=e, resid=prefill(dtype, 3))
    call(M_GRAD, dtype, a)
    assert same_bits(a["resid"], (w3 * y3).astype(T)), "Poisson gradient with exp(eta) underflowed"
    p = dict(kind=POISSON, n=3, K=1, nb=3, y=y3, w=w3, eta=e, resid=a["resid"].copy(), off=np.zeros(3, dtype=T), hmin=HMIN,
             hess=prefill(dtype, 3), irls_resid=prefill(dtype, 3), irls_y=prefill(dtype, 3))
    call(M_PREPARE, dtype, p)
    hmin = T(HMIN)
    with np.errstate(all="ignore"):
        assert (p["hess"] == hmin).all() and same_bits(p["irls_resid"], (p["resid"] / hmin).astype(T))
        assert same_bits(p["irls_y"], (p["irls_resid"] + e - T(0)).astype(T))
        q = copy_inputs(p)
        call(M_NULL, dtype, q)
        # the null step's sums use the raised value: 3 hmin and sum hmin (z + eta - off), three terms: within gamma_3 + the product
        assert abs(float(q["sums"][0]) - 3 * float(hmin)) <= 4 * UNIT[dtype] * 3 * float(hmin)
        t = hmin * (p["irls_resid"] + e)
        assert abs(float(q["sums"][1]) - float(np.sum(t.astype(np.float64)))) <= 4 * UNIT[dtype] * float(np.abs(t).sum())


# ---- REL_CHANGE ----------------------------------------------------------------------------------------------------------------------
def rel_expected(T, a, prev):
    with np.errstate(all="ignore"):
        d = np.abs(a - prev)
        r = np.where(prev > 0, d / prev, np.where(d > 0, T(1e30), T(0))).astype(T)
        r = np.where(np.isnan(r) | np.isnan(d), T(1e30), r).astype(T)
        return max(T(0), r.max())


def rel_cases(dtype):
    T = NP_TYPE[dtype]
    out = []
    for n in N_LIST:
        rng = _rng("rel %s %d" % (dtype, n))
        prev = rng.uniform(0.5, 1.5, size=n).astype(T)
        a = (prev * (1 + rng.uniform(-0.01, 0.01, size=n))).astype(T)
        a[n - 1] = prev[n - 1] * T(1.25)                          # the largest change sits in the tail element
        out.append(("n%d-tail" % n, a, prev))
        if n > 64:
            a2 = a.copy()
            a2[n - 1] = prev[n - 1]
            a2[63] = prev[63] * T(1.5)
            out.append(("n%d-lane63" % n, a2, prev))
    z, one = np.zeros(70, dtype=T), np.ones(70, dtype=T)
    out.append(("zeros", z, z.copy()))
    pa = z.copy()
    pa[65] = T(2.0 ** -20)
    out.append(("prev0-a-positive", pa, z.copy()))
    na = one.copy()
    na[3] = np.nan
    out.append(("nan-in-a", na, one.copy()))
    out.append(("nan-in-prev", one.copy(), na.copy()))
    ia = one.copy()
    ia[69] = np.inf
    out.append(("inf-minus-inf", ia, ia.copy()))
    out.append(("all-equal", (one * T(0.3)).astype(T), (one * T(0.3)).astype(T)))
    neg = one.copy()
    neg[5] = -1
    out.append(("negative-prev", one.copy(), neg))
    return out


def run_rel_change(call, dtype):
    T = NP_TYPE[dtype]
    for name, x, prev in rel_cases(dtype):
        a = dict(n=x.size, wts=x.copy(), prev=prev.copy())
        d = twice(call, M_REL, dtype, a)
        want = rel_expected(T, x, prev)
        assert same_bits(d["sums"][15:16], np.array([want], dtype=T)), "rel_change %s %s: %r, expected %r (a sentinel of %g was in the slot)" % (
            name, dtype, d["sums"][15], want, SENTINEL)
        assert same_bits(d["prev"], x), "rel_change %s: prev is not a copy of a" % name
        assert same_bits(d["wts"], x)
        check_sums_footprint(M_REL, dtype, d["sums"])
        if name in ("all-equal", "zeros"):
            assert bits(d["sums"][15:16])[0] == 0


# ---- the exact leg --------------------------------------------------------------------------------------------------------------------
def position_class(n):
    i = np.arange(n)
    return ((i % 64 == 63).astype(int) + (i % 256 == 255) + (i % STRIDE == STRIDE - 1) + (i >= STRIDE) + (i == n - 1) + (i % 2))


def exact_inputs(mode, dtype, n, K=1):
    """Small integers (see the module docstring); n counts elements (rows for MULTI_LOSS2)."""
    T = NP_TYPE[dtype]
    rng = _rng("glm exact %s %s %d %d" % (MODE_NAME[mode], dtype, n, K))
    w = (2 ** position_class(n)).astype(np.int64)
    I = lambda lo, hi, size=n: rng.randint(lo, hi + 1, size=size).astype(np.int64)      # noqa: E731
    a = dict(kind=GAUSSIAN, n=n, K=1, nb=n)
    if mode in (M_PREPARE, M_NULL):
        a.update(y=I(-3, 3), w=w, eta=2 * I(-1, 1), off=2 * I(-1, 1), resid=w * (2 * I(0, 2) + 1), hmin=HMIN)   # (z + eta - off is odd)
    elif mode == M_WEIGHTS:
        a.update(hess=w, irls_y=2 * I(-1, 1) + 1, irls_resid=I(-3, 2) * 2, hess_sum=1024.0, shift=1.0)
    elif mode == M_FINISH:
        a.update(y=2 * I(-2, 2), w=w, irls_y=I(-2, 2), off=I(-2, 2), irls_resid=2 * I(-1, 1), shift=3.0)
    elif mode == M_GRAD:
        a.update(y=2 * I(-2, 2) + 1, w=w, eta=2 * I(-2, 2))
    elif mode == M_LOSS:
        a.update(y=I(-1, 0), w=w, eta=2 * I(1, 2))
    elif mode == M_LOSS2:
        a.update(y=I(-1, 0), w=w, wb=(2 ** (np.arange(n) % 3)).astype(np.int64), eta=2 * I(1, 2) + 3, off=I(0, 1) * 0 - 1, b0=-2.0)
    elif mode == M_MLOSS2:
        e = 2 * I(1, 2, (K, n))
        y = I(-1, 0, (K, n))
        if K in (3, 7):                                          # the row's sum of 0.5 e^2 - y e a multiple of K: l = a / K is an integer
            e[K - 1] = 2
            S = (e[:K - 1] ** 2 // 2 - y[:K - 1] * e[:K - 1]).sum(axis=0)
            y[K - 1] = ((S + 2) * ((K + 1) // 2)) % K              # (K + 1) / 2 is the inverse of 2 modulo K
        b0v = np.arange(K) % 3 - 1
        off = I(-1, 1, (K, n))
        a.update(kind=GAUSSIAN, n=n * K, nb=n, K=K, y=y.reshape(-1), w=w, wb=(2 ** (np.arange(n) % 3)).astype(np.int64),
                 eta=(e - b0v[:, None] - off).reshape(-1), off=off.reshape(-1), b0v=b0v)
    elif mode == M_SET_ETA:
        a.update(off=I(-99, 99), b0=7.0)
    elif mode == M_DOT:
        a.update(resid=w * 2, resid_prev=w, eta=I(1, 3) + 4, eta_prev=I(0, 3))
    out = {k: (np.ascontiguousarray(v).astype(T) if isinstance(v, np.ndarray) else v) for k, v in a.items()}
    for name in OUTPUTS[mode]:
        if name not in out:
            out[name] = prefill(dtype, out["n"])
    return out


def run_exact(call, mode, dtype, n, K=1):
    """Integer inputs: outputs bit for bit against an int64 reference."""
    T = NP_TYPE[dtype]
    a = exact_inputs(mode, dtype, n, K)
    d = twice(call, mode, dtype, a)
    g = {k: (v.astype(np.int64) if isinstance(v, np.ndarray) and k in INPUTS.get(mode, ()) + ("b0v",) else v) for k, v in a.items()}
    elem, sums, scale = {}, [], 1

    def eq(name, ref):
        assert np.array_equal(d[name], ref.astype(T)), "%s n=%d: %s differs from the integer reference at %s" % (
            MODE_NAME[mode], n, name, np.flatnonzero(d[name] != ref.astype(T))[:4].tolist())

    if mode in (M_PREPARE, M_NULL):
        z = g["resid"] // g["w"]
        iy = z + g["eta"] - g["off"]
        if mode == M_PREPARE:
            elem, sums = dict(hess=g["w"], irls_resid=z, irls_y=iy), [g["w"]]
        else:
            sums = [g["w"], g["w"] * iy]
    elif mode == M_WEIGHTS:
        scale = 1024
        ri = g["irls_resid"] + 1
        assert np.array_equal(d["wts"].astype(np.float64) * 1024, g["hess"].astype(np.float64))
        elem = dict(irls_resid=ri)
        sums = [g["hess"] * g["irls_y"], g["hess"] * g["irls_y"] ** 2, g["hess"] * ri]
    elif mode == M_FINISH:
        e = g["irls_y"] + g["off"] - g["irls_resid"] + 3
        elem = dict(eta=e, resid=g["w"] * (g["y"] - e))
    elif mode == M_GRAD:
        elem = dict(resid=g["w"] * (g["y"] - g["eta"]))
    elif mode == M_LOSS:
        sums = [g["w"] * (g["eta"] ** 2 // 2 - g["y"] * g["eta"])]
    elif mode == M_LOSS2:
        e = g["eta"] - 2 + g["off"]
        l = e ** 2 // 2 - g["y"] * e
        assert (e % 2 == 0).all()
        sums = [g["w"] * l, g["wb"] * l]
    elif mode == M_MLOSS2:
        E = (g["eta"].reshape(K, n) + g["b0v"][:, None] + g["off"].reshape(K, n))
        assert (E % 2 == 0).all()
        tot = (E ** 2 // 2 - g["y"].reshape(K, n) * E).sum(axis=0)
        assert (tot % K == 0).all()
        sums = [g["w"] * (tot // K), g["wb"] * (tot // K)]
    elif mode == M_SET_ETA:
        elem = dict(eta=g["off"] + 7)
    elif mode == M_DOT:
        sums = [(g["resid"] - g["resid_prev"]) * (g["eta"] - g["eta_prev"])]
    for name, ref in elem.items():
        eq(name, ref)
    for k in INPUTS[mode]:
        if k not in OUTPUTS[mode]:
            assert same_bits(d[k], a[k]), "%s changed its input %s" % (MODE_NAME[mode], k)
    if mode in NSUMS:
        check_sums_footprint(mode, dtype, d["sums"])
        for q, t in enumerate(sums):
            assert (t != 0).all() and np.abs(t).sum() < 2 ** 24, (MODE_NAME[mode], n, q, int(np.abs(t).sum()))
            assert float(d["sums"][q]) * scale == float(t.sum()), "%s n=%d K=%d: sums[%d] = %r, the integer reference is %d / %d" % (
                MODE_NAME[mode], n, K, q, d["sums"][q], t.sum(), scale)
    return {}


def run_moves(call, dtype):
    """GATHER and SCATTER on integers: bit for bit, dst untouched wherever nothing is written (everywhere for cnt = 0)."""
    T = NP_TYPE[dtype]
    for cnt in MOVE_CNT:
        rng = _rng("glm moves %s %d" % (dtype, cnt))
        N = 1500
        table = (np.arange(N) + 1).astype(T)
        idx = rng.randint(0, N, size=max(cnt, 1)).astype(np.int32)
        if cnt:
            idx[cnt - 1] = N - 1
        a = dict(cnt=cnt, src=table, src_elems=N, idx=idx, dst=prefill(dtype, cnt + 3), dst_elems=cnt + 3)
        call(M_GATHER, dtype, a)
        assert np.array_equal(a["dst"][:cnt], table[idx[:cnt]]) and is_prefill(a["dst"][cnt:]).all(), "gather cnt=%d" % cnt
        perm = rng.permutation(N)[:max(cnt, 1)].astype(np.int32)
        if cnt and N - 1 not in perm[:cnt]:
            perm[cnt - 1] = N - 1
        src = (np.arange(max(cnt, 1)) + 1).astype(T)
        b = dict(cnt=cnt, src=src, src_elems=max(cnt, 1), idx=perm, dst=prefill(dtype, N), dst_elems=N)
        call(M_SCATTER, dtype, b)
        want = prefill(dtype, N)
        want[perm[:cnt]] = src[:cnt]
        assert same_bits(b["dst"], want), "scatter cnt=%d" % cnt
