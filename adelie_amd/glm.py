"""GLM plugin surface — mirrors ``adelie.glm`` for the families on the grpnet hot path.

Reference: ``adelie/glm.py:40-55`` (weight normalisation), ``:83-196`` (``binomial``), ``:374-453``
(``gaussian`` with its ``opt`` flag), and the C++ classes ``glm/glm_base.ipp:23-37``,
``glm/glm_gaussian.ipp:15-63``, ``glm/glm_binomial.ipp:14-99``.

The objects below are host-side descriptors: they carry ``y``/``weights`` and the closed-form
member functions (written in numpy, used by the Python preamble of ``grpnet`` and by ``cv_grpnet``).
Inside the path solver the same functions run as fused HIP elementwise kernels, selected by
``core_kind`` (``adelie_hip_glm_kind`` in ``include/adelie_hip.h``).
"""
import numpy as np

from . import _abi
from . import configs as _configs


def _coerce_dtype(y, dtype):
    """Reference ``glm.py:12-33`` (with ``np.asarray`` instead of numpy-1 ``copy=False``)."""
    valid = (np.dtype("float32"), np.dtype("float64"))
    y = np.asarray(y, order="C")
    if dtype is None:
        if y.dtype not in valid:
            raise RuntimeError(
                "y must have an underlying type of np.float32 or np.float64, "
                "or dtype must be explicitly specified."
            )
        dtype = y.dtype.type
    else:
        if np.dtype(dtype) not in valid:
            raise RuntimeError("dtype must be either np.float32 or np.float64.")
        dtype = np.dtype(dtype).type
    return y.astype(dtype, copy=False), dtype


class GlmBase:
    """Base class of every family, and the plugin surface for user-defined ones (reference ``GlmBase{32,64}``,
    ``glm/glm_base.hpp:19-93``, Python-subclassable through ``py_glm.cpp:8-92``).

    A user-defined single-response family subclasses :class:`GlmBase64` (or :class:`GlmBase32`), calls
    ``GlmBase64.__init__(self, name, y, weights)`` and implements ``gradient(eta, grad)`` (the NEGATIVE gradient of the
    loss, written in place), ``hessian(eta, grad, hess)``, ``loss(eta)`` and ``loss_full()``; ``inv_hessian_gradient`` and
    ``inv_link`` are optional.  ``grpnet`` runs such a family through the IRLS solver on the device and calls these methods
    on host n-vectors once per IRLS iteration (``adelie_hip_glm_callbacks``)."""

    is_multi = False
    opt = False

    def __init__(self, name, y, weights):
        self.name = name
        self.y = y
        self.weights = weights

    def gradient(self, eta, grad):
        raise NotImplementedError("gradient() must be implemented by the GLM subclass.")

    def hessian(self, eta, grad, hess):
        raise NotImplementedError("hessian() must be implemented by the GLM subclass.")

    def loss(self, eta):
        raise NotImplementedError("loss() must be implemented by the GLM subclass.")

    def loss_full(self):
        raise NotImplementedError("loss_full() must be implemented by the GLM subclass.")

    def inv_link(self, eta, out):
        raise NotImplementedError("inv_link() must be implemented by the GLM subclass.")

    # glm_base.ipp:23-37
    def inv_hessian_gradient(self, eta, grad, hess, inv_hess_grad):
        hmin = _configs.Configs.hessian_min
        inv_hess_grad[...] = grad / (np.maximum(hess, 0) + hmin * (hess <= 0))


class GlmBase64(GlmBase):
    pass


class GlmBase32(GlmBase):
    pass


class glm_base:
    """Reference ``glm.py:36-55``."""

    def __init__(self, y, weights, dtype):
        self.y = np.array(y, copy=True, dtype=dtype)
        self.dtype = dtype
        if len(y.shape) != 1:
            raise RuntimeError("y must be 1-dimensional.")
        n = y.shape[0]
        if weights is not None:
            weights = np.asarray(weights)
            if weights.shape != (n,):
                raise RuntimeError("y and weights must have same length.")
            weights_sum = np.sum(weights)
            if not np.allclose(weights_sum, 1):
                weights = weights / weights_sum
        else:
            weights = np.full(n, 1 / n, dtype=dtype)
        self.weights = np.array(weights, copy=True, dtype=dtype)

    # glm_base.ipp:23-37
    def inv_hessian_gradient(self, eta, grad, hess, inv_hess_grad):
        hmin = self.dtype(_configs.Configs.hessian_min)
        inv_hess_grad[...] = grad / (np.maximum(hess, 0) + hmin * (hess <= 0))


def _mixin(dtype):
    return GlmBase64 if np.dtype(dtype) == np.float64 else GlmBase32


def gaussian(y, *, weights=None, dtype=None, opt: bool = True):
    """Gaussian family (reference ``adelie.glm.gaussian``, ``glm.py:374-453``)."""
    y, dtype = _coerce_dtype(y, dtype)

    class _gaussian(glm_base, _mixin(dtype)):
        name = "gaussian"

        def __init__(self):
            self.opt = opt
            glm_base.__init__(self, y, weights, dtype)
            self.core_kind = _abi.GLM_GAUSSIAN if opt else _abi.GLM_GAUSSIAN_IRLS

        # glm_gaussian.ipp:15-63
        def gradient(self, eta, grad):
            grad[...] = self.weights * (self.y - eta)

        def hessian(self, eta, grad, hess):
            hess[...] = self.weights

        def loss(self, eta):
            return np.sum(self.weights * (0.5 * np.square(eta) - self.y * eta))

        def loss_full(self):
            return -0.5 * np.sum(np.square(self.y) * self.weights)

        def inv_link(self, eta, out):
            out[...] = eta

        def reweight(self, weights=None):
            w = self.weights if weights is None else weights
            return gaussian(y=y, weights=w, dtype=dtype, opt=opt)

    return _gaussian()


class multiglm_base:
    """Reference ``glm.py:57-80``: ``y`` is ``(n, K)``, one weight per observation."""

    def __init__(self, y, weights, dtype):
        self.y = np.array(y, copy=True, dtype=dtype)
        self.dtype = dtype
        if len(y.shape) != 2:
            raise RuntimeError("y must be 2-dimensional.")
        n = y.shape[0]
        if weights is not None:
            weights = np.asarray(weights)
            if weights.shape != (n,):
                raise RuntimeError("y rows and weights must have same length.")
            weights_sum = np.sum(weights)
            if not np.allclose(weights_sum, 1):
                weights = weights / weights_sum
        else:
            weights = np.full(n, 1 / n, dtype=dtype)
        self.weights = np.array(weights, copy=True, dtype=dtype)


def multigaussian(y, *, weights=None, dtype=None, opt: bool = True):
    """MultiGaussian family (reference ``adelie.glm.multigaussian``, ``glm.py:456-535``; arithmetic
    ``glm_multigaussian.ipp:15-63``): ``loss = (1/K) sum_i w_i (||eta_i||^2 / 2 - y_i . eta_i)``.

    Only the optimised route (``opt=True``: the Gaussian naive solver on ``[1 (x) I_K, X (x) I_K]``) is on the device
    path; the IRLS route for multi-response GLMs is not."""
    y, dtype = _coerce_dtype(y, dtype)
    if not opt:
        raise NotImplementedError("adelie_amd.glm.multigaussian: only opt=True is on the device path.")

    class _multigaussian(multiglm_base, _mixin(dtype)):
        name = "multigaussian"
        is_multi = True

        def __init__(self):
            self.opt = opt
            multiglm_base.__init__(self, y, weights, dtype)

        def gradient(self, eta, grad):
            grad[...] = (self.weights[:, None] * (self.y - eta)) / self.y.shape[1]

        def hessian(self, eta, grad, hess):
            hess[...] = self.weights[:, None] / self.y.shape[1]

        def loss(self, eta):
            return np.sum(self.weights * np.sum(0.5 * np.square(eta) - self.y * eta, axis=1)) / self.y.shape[1]

        def loss_full(self):
            return -0.5 * np.sum(np.square(self.y) * self.weights[:, None]) / self.y.shape[1]

        def inv_link(self, eta, out):
            out[...] = eta

        def reweight(self, weights=None):
            w = self.weights if weights is None else weights
            return multigaussian(y=y, weights=w, dtype=dtype, opt=opt)

    return _multigaussian()


def multinomial(y, *, weights=None, dtype=None):
    """Multinomial family (reference ``adelie.glm.multinomial``, ``glm.py:538-618``; arithmetic ``glm_multinomial.ipp:21-115``):
    ``loss = (1/K) sum_i w_i (-y_i . eta_i + log sum_k exp eta_ik)``, diagonal majorant ``2 K^-1 W P (1 - P)`` as Hessian."""
    y, dtype = _coerce_dtype(y, dtype)
    if y.ndim == 2 and y.shape[1] <= 1:
        raise RuntimeError("adelie_core: y must have at least 2 columns (classes).")

    class _multinomial(multiglm_base, _mixin(dtype)):
        name = "multinomial"
        is_multi = True
        opt = False

        def __init__(self):
            multiglm_base.__init__(self, y, weights, dtype)
            self.core_kind = _abi.GLM_MULTINOMIAL

        def _prob(self, eta):
            e = np.exp(eta - np.max(eta, axis=1)[:, None])
            return e / np.sum(e, axis=1)[:, None]

        def gradient(self, eta, grad):
            grad[...] = (self.y - self._prob(eta)) * self.weights[:, None] / self.y.shape[1]

        def hessian(self, eta, grad, hess):
            K = self.y.shape[1]
            w = self.weights[:, None]
            h = self.y * w / K - grad
            hess[...] = h * (2 * (1 - K * (h / (w + (w <= 0)))))

        def inv_hessian_gradient(self, eta, grad, hess, inv_hess_grad):
            hmin = self.dtype(_configs.Configs.hessian_min)
            inv_hess_grad[...] = grad / (np.maximum(hess, 0) + hmin * (hess <= 0))

        def loss(self, eta):
            es = eta - np.max(eta, axis=1)[:, None]
            return np.sum(self.weights * (-np.sum(self.y * es, axis=1) + np.log(np.sum(np.exp(es), axis=1)))) / self.y.shape[1]

        def loss_full(self):
            with np.errstate(divide="ignore", invalid="ignore"):
                ly = np.log(self.y)
                t = np.where(np.isfinite(ly), self.y * ly, 0.0)
            return self.dtype(-np.sum(np.sum(t, axis=1) * self.weights) / self.y.shape[1])

        def inv_link(self, eta, out):
            out[...] = self._prob(eta)

        def reweight(self, weights=None):
            w = self.weights if weights is None else weights
            return multinomial(y=y, weights=w, dtype=dtype)

    return _multinomial()


def poisson(y, *, weights=None, dtype=None):
    """Poisson family, log link (reference ``adelie.glm.poisson``, ``glm.py:621-697``; arithmetic ``glm_poisson.ipp:14-58``)."""
    y, dtype = _coerce_dtype(y, dtype)

    class _poisson(glm_base, _mixin(dtype)):
        name = "poisson"

        def __init__(self):
            glm_base.__init__(self, y, weights, dtype)
            self.core_kind = _abi.GLM_POISSON

        def gradient(self, eta, grad):
            grad[...] = self.weights * (self.y - np.exp(eta))

        def hessian(self, eta, grad, hess):
            hess[...] = self.weights * self.y - grad

        def loss(self, eta):
            mx = np.finfo(self.dtype).max
            return np.sum(self.weights * (np.minimum(-eta, mx) * self.y + np.exp(eta)))

        def loss_full(self):
            mx = np.finfo(self.dtype).max
            with np.errstate(divide="ignore", invalid="ignore"):
                t = np.minimum(-np.log(self.y), mx) * self.y
            return self.dtype(np.sum(self.weights * (np.where(self.y > 0, t, 0.0) + self.y)))

        def inv_link(self, eta, out):
            out[...] = np.exp(eta)

        def reweight(self, weights=None):
            w = self.weights if weights is None else weights
            return poisson(y=y, weights=w, dtype=dtype)

    return _poisson()


def _binomial_probit(y, weights, dtype):
    """Binomial family, probit link (reference ``glm_binomial.ipp:100-190``)."""
    from scipy.special import erf

    class _probit(glm_base, _mixin(dtype)):
        name = "binomial_probit"

        def __init__(self):
            glm_base.__init__(self, y, weights, dtype)
            self.core_kind = _abi.GLM_BINOMIAL_PROBIT

        @staticmethod
        def _cdf(x):
            return 0.5 * (1 + erf(x / np.sqrt(2)))

        @staticmethod
        def _pdf(x):
            return np.exp(-0.5 * np.square(x)) / np.sqrt(2 * np.pi)

        def gradient(self, eta, grad):
            mx = np.finfo(self.dtype).max
            c = self._cdf(eta)
            with np.errstate(divide="ignore"):
                grad[...] = self.weights * self._pdf(eta) * (
                    self.y * np.minimum(1 / c, mx) - (1 - self.y) * np.minimum(1 / (1 - c), mx))

        def hessian(self, eta, grad, hess):
            mx = np.finfo(self.dtype).max
            c = self._cdf(eta)
            with np.errstate(divide="ignore"):
                hess[...] = self.weights * (
                    self.y * np.minimum(1 / np.square(c), mx) + (1 - self.y) * np.minimum(1 / np.square(1 - c), mx)
                ) * np.square(self._pdf(eta)) + eta * grad

        def loss(self, eta):
            mx = np.finfo(self.dtype).max
            c = self._cdf(eta)
            with np.errstate(divide="ignore"):
                return -np.sum(self.weights * (
                    self.y * np.maximum(np.log(c), -mx) + (1 - self.y) * np.maximum(np.log(1 - c), -mx)))

        def loss_full(self):
            with np.errstate(divide="ignore", invalid="ignore"):
                ly, l1y = np.log(self.y), np.log(1 - self.y)
                t1, t2 = self.weights * self.y * ly, self.weights * (1 - self.y) * l1y
            return self.dtype(-np.sum(t1[np.isfinite(ly)]) - np.sum(t2[np.isfinite(l1y)]))

        def inv_link(self, eta, out):
            out[...] = self._cdf(eta)

        def reweight(self, weights=None):
            w = self.weights if weights is None else weights
            return _binomial_probit(y, w, dtype)

    return _probit()


def binomial(y, *, weights=None, link: str = "logit", dtype=None):
    """Binomial family, logit or probit link (reference ``adelie.glm.binomial``, ``glm.py:83-196``)."""
    y, dtype = _coerce_dtype(y, dtype)
    if link == "probit":
        return _binomial_probit(y, weights, dtype)
    if link != "logit":
        raise RuntimeError("link must be one of 'logit' or 'probit'.")

    class _binomial(glm_base, _mixin(dtype)):
        name = "binomial_logit"

        def __init__(self):
            glm_base.__init__(self, y, weights, dtype)
            self.core_kind = _abi.GLM_BINOMIAL_LOGIT

        # glm_binomial.ipp:37-99
        def gradient(self, eta, grad):
            grad[...] = self.weights * (self.y - 1 / (1 + np.exp(-eta)))

        def hessian(self, eta, grad, hess):
            w = self.weights
            h = w * self.y - grad
            hess[...] = (h * (w - h)) / (w + (w <= 0))

        def loss(self, eta):
            mx = np.finfo(self.dtype).max
            return np.sum(self.weights * (
                ((eta > 0).astype(self.dtype) - self.y) * np.clip(eta, -mx, mx)
                + np.log1p(np.exp(-np.abs(eta)))
            ))

        def loss_full(self):
            # glm_binomial.ipp:14-33: non-finite logs are skipped
            with np.errstate(divide="ignore", invalid="ignore"):
                ly = np.log(self.y)
                l1y = np.log(1 - self.y)
                t1 = self.weights * self.y * ly
                t2 = self.weights * (1 - self.y) * l1y
            loss = 0.0
            loss -= np.sum(t1[np.isfinite(ly)])
            loss -= np.sum(t2[np.isfinite(l1y)])
            return self.dtype(loss)

        def inv_link(self, eta, out):
            out[...] = 1 / (1 + np.exp(-eta))

        def reweight(self, weights=None):
            w = self.weights if weights is None else weights
            return binomial(y=y, weights=w, dtype=dtype)

    return _binomial()


# ------------------------------------------------------------------------------------------------------------------------
# Cox proportional hazards (reference ``adelie.glm.cox``, ``glm.py:199-371``; arithmetic ``glm_cox.ipp:356-514, 649-748``)
#
# Every quantity lives in one of three orders: the caller's row order, "stop order" (rows sorted by (stratum, stop), stable)
# and "start order" (sorted by (stratum, start), stable).  Strata occupy the same contiguous segment in both sorted orders.
# A tie group is a run of equal stop times inside a stratum (stop order).  The scans below are truly segmented: a sum never
# crosses a stratum (or tie group) boundary, so a small stratum after a large one keeps all its digits.

def _seg_cumsum(x, first):
    """Inclusive prefix sums of ``x`` restarted wherever ``first`` is True (Hillis-Steele doubling: O(n log L) for segments
    of length <= L, exact segmentation; the association is a fixed tree)."""
    x = np.array(x, dtype=np.float64, copy=True)
    n = x.shape[0]
    # seg_lo[i]: position of the first element of i's segment
    seg_lo = np.maximum.accumulate(np.where(first, np.arange(n), 0)) if n else np.zeros(0, dtype=np.int64)
    pos = np.arange(n)
    d = 1
    while d < n:
        m = pos[d:] - d >= seg_lo[d:]
        if not m.any():
            break
        add = np.where(m, x[:-d], 0.0)
        x[d:] = x[d:] + add
        d *= 2
    return x


class _CoxOrders:
    """The weight-free part of a Cox family: sort orders, tie groups and the search positions of the at-risk sums.  Computed
    once per (start, stop, strata) and shared by every ``reweight`` of the family."""

    def __init__(self, start, stop, strata):
        n = stop.shape[0]
        self.n = n
        self.n_strata = int(strata.max()) + 1 if n else 0
        self.to = np.lexsort((stop, strata))           # stop order (stable)
        self.so = np.lexsort((start, strata))          # start order (stable)
        st = strata[self.to]
        self.stratum_sorted = st
        counts = np.bincount(strata, minlength=self.n_strata)
        self.outer = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        lo = self.outer[st]                            # segment [lo, hi) of each sorted position
        hi = self.outer[st + 1]
        pos = np.arange(n)
        self.seg_first = pos == lo
        self.seg_last = pos == hi - 1
        stop_to = stop[self.to]
        start_so = start[self.so]
        gflag = self.seg_first.copy()
        gflag[1:] |= stop_to[1:] != stop_to[:-1]
        self.gflag = gflag
        self.gid = np.cumsum(gflag) - 1
        gstarts = np.flatnonzero(gflag)
        gends = np.append(gstarts[1:], n)
        self.gstarts = gstarts
        self.gstart = gstarts[self.gid]
        self.gend = gends[self.gid]
        # at-risk sums need, per stop position q, the first start position of its stratum with start >= stop_to[q]; the
        # start-order term needs, per start position, the first stop position of its stratum with stop > start_so[q].
        # Both are searches on the key (stratum, rank of the time among all start and stop times), monotone in both orders.
        _, ranks = np.unique(np.concatenate([stop_to, start_so]), return_inverse=True)
        U = np.int64(ranks.max() + 2 if n else 1)
        key_to = st.astype(np.int64) * U + ranks[:n]
        key_so = st.astype(np.int64) * U + ranks[n:]
        b = np.searchsorted(key_so, key_to, side="left")
        self.bpos = np.where(b < hi, b, -1)           # -1: no start time in the stratum is >= stop_to[q]
        ub = np.searchsorted(key_to, key_so, side="right")
        self.ub_m1 = np.where(ub > lo, ub - 1, -1)     # last stop position with stop <= start_so[q]; -1: none


def cox(start, stop, status, *, strata=None, weights=None, tie_method: str = "efron", dtype=None):
    """Cox family (reference ``adelie.glm.cox``, ``glm.py:199-371``):

    ``loss(eta) = -sum_i w_i d_i eta_i + sum_i wbar_i d_i log(sum_{k in R(t_i)} w_k e^eta_k - sigma_i sum_{k in H(t_i)} w_k e^eta_k)``

    summed over strata, with ``R(u) = {k : s_k < u <= t_k}``, ``H(u)`` the events at ``u`` with non-zero weight, ``wbar`` their
    average weight and ``sigma`` the Efron scales (zero for Breslow).  The numpy members below serve the Python preamble,
    ``diagnostic``, the tests, and ``cv_grpnet``'s fold losses on plugin designs; inside ``grpnet`` the family is evaluated on
    the device (``kernels_cox.hip``) from a handle the library builds on first use (``_device_handle``), and ``cv_grpnet`` on a
    native design takes a fold's losses under the full-data and the training family from ``X.cox_path_losses``: every lambda
    in one batched device evaluation from the same handles, the etas never leaving HBM."""
    status, dtype = _coerce_dtype(status, dtype)
    return _cox_make(start, stop, status, strata, weights, tie_method, dtype, None)


def _cox_make(start, stop, status, strata, weights, tie_method, dtype, orders):
    n = status.shape[0] if status.ndim == 1 else -1
    if status.ndim != 1:
        raise RuntimeError("y must be 1-dimensional.")
    start = np.array(start, copy=True, dtype=dtype)
    stop = np.array(stop, copy=True, dtype=dtype)
    if strata is None:
        strata = np.zeros(n, dtype=int)
    strata = np.array(strata, copy=True, dtype=int)
    # glm_cox.ipp:600-645
    if start.shape != (n,):
        raise RuntimeError("start must be (n,) where status is (n,).")
    if stop.shape != (n,):
        raise RuntimeError("stop must be (n,) where status is (n,).")
    if strata.shape != (n,):
        raise RuntimeError("strata must be (n,) where status is (n,).")
    if n and strata.min() < 0:
        raise RuntimeError("strata must take values in {0, ..., M-1}.")
    if tie_method not in ("efron", "breslow"):
        raise RuntimeError("Invalid tie method: " + str(tie_method))
    if orders is None:
        orders = _CoxOrders(start, stop, strata)

    class _cox(glm_base, _mixin(dtype)):
        name = "cox"

        def __init__(self):
            glm_base.__init__(self, status, weights, dtype)
            self.status = self.y
            self.start = start
            self.stop = stop
            self.strata = strata
            self.tie_method = tie_method
            self.core_kind = _abi.GLM_COX
            self._orders = orders
            self._handles = {}
            self._pack_weights()

        def _pack_weights(self):
            """The weight-dependent part of the pack (stop order): event indicators with non-zero weight, tie sizes, averaged
            weights ``wbar`` and the tie-breaking scales (glm_cox.ipp:151-264, 302-354)."""
            o = self._orders
            w_to = self.weights.astype(np.float64)[o.to]
            d_to = self.status.astype(np.float64)[o.to]
            ind = d_to * (w_to != 0)
            if o.n:
                size = np.add.reduceat(ind, o.gstarts)[o.gid] * ind
                wsum = np.add.reduceat(w_to * ind, o.gstarts)[o.gid] * ind
            else:
                size = wsum = np.zeros(0)
            wbar = np.divide(wsum, size, out=np.zeros_like(wsum), where=size > 0)
            if self.tie_method == "breslow" or not o.n:
                scale = np.zeros(o.n)
            else:
                cum = np.cumsum(ind)
                k = cum - ind - (cum - ind)[o.gstart]    # events with non-zero weight before q in its tie group
                scale = np.divide(k * ind, size, out=np.zeros(o.n), where=size > 0)
            self._ind, self._size, self._wbar, self._scale = ind, size, wbar, scale
            self._dw = d_to * wbar

        def _risk_total(self, eta):
            """z = w exp(eta - c) with c = max eta (row order) and the risk totals of the events (stop order):
            sum_{k in R(t_q)} z_k - sigma_q sum_{k in H(t_q)} z_k."""
            o = self._orders
            eta = np.asarray(eta, dtype=np.float64)
            c = eta.max()
            z = self.weights.astype(np.float64) * np.exp(eta - c)
            z_to, z_so = z[o.to], z[o.so]
            s_stop = _seg_cumsum(z_to[::-1], o.seg_last[::-1])[::-1]     # sum over stop order from q to the stratum's end
            s_start = _seg_cumsum(z_so[::-1], o.seg_last[::-1])[::-1]
            ties = np.add.reduceat(z_to * self._ind, o.gstarts)[o.gid] * self._ind
            risk = s_stop[o.gstart] - np.where(o.bpos >= 0, s_start[np.maximum(o.bpos, 0)], 0.0)
            return z, risk - self._scale * ties, c

        def _risk_scaled(self, v, sc):
            """Row order: sum over the events i with z_row in R(t_i) of v_i, minus the tie term sc_i v_i over the row's own
            event tie (glm_cox.ipp:439-446): the factor of z (gradient) or z^2 (Hessian)."""
            o = self._orders
            P = _seg_cumsum(v, o.seg_first)
            tie = np.add.reduceat(v * sc * self._ind, o.gstarts)[o.gid] * self._ind
            acc = np.empty(o.n)
            acc[o.to] = P[o.gend - 1] - tie
            acc[o.so] -= np.where(o.ub_m1 >= 0, P[np.maximum(o.ub_m1, 0)], 0.0)
            return acc

        def _grad_hess(self, eta, want_hess):
            w = self.weights.astype(np.float64)
            wd = w * self.status.astype(np.float64)
            if self._orders.n == 0:
                return np.zeros(0), np.zeros(0)
            z, rt, _ = self._risk_total(eta)
            nz = self._dw != 0
            v = np.divide(self._dw, rt, out=np.zeros_like(rt), where=nz)
            grad = wd - z * self._risk_scaled(v, self._scale)
            if not want_hess:
                return grad, None
            v2 = np.divide(v, rt, out=np.zeros_like(rt), where=nz)
            return grad, wd - grad - z * z * self._risk_scaled(v2, self._scale * (2 - self._scale))

        def gradient(self, eta, grad):
            grad[...] = self._grad_hess(eta, False)[0]

        def hessian(self, eta, grad, hess):
            # (recomputed from eta: `grad` is the gradient at eta, as for every family)
            hess[...] = self._grad_hess(eta, True)[1]

        def loss(self, eta):
            if self._orders.n == 0:
                return self.dtype(0)
            mx = np.finfo(self.dtype).max
            _, rt, c = self._risk_total(eta)
            with np.errstate(divide="ignore", invalid="ignore"):
                lg = np.maximum(np.log(np.maximum(rt, 0)), -mx)
            wd = self.weights.astype(np.float64) * self.status
            return -np.sum(wd * (np.asarray(eta, dtype=np.float64) - c)) + np.sum(np.where(self._dw != 0, self._dw * lg, 0.0))

        def loss_full(self):
            mx = np.finfo(self.dtype).max
            with np.errstate(divide="ignore", invalid="ignore"):
                lg = np.maximum(np.log(self._size * self._wbar * (1 - self._scale)), -mx)
            return self.dtype(np.sum(np.where(self._dw != 0, self._dw * lg, 0.0)))

        def inv_link(self, eta, out):
            out[...] = np.exp(eta)

        def reweight(self, weights=None):
            w = self.weights if weights is None else weights
            return _cox_make(self.start, self.stop, self.status, self.strata, w, self.tie_method, dtype, self._orders)

        def _device_handle(self, device):
            """``adelie_hip_glm_cox`` of this family on ``device``, created on first use and kept with the family (immutable:
            every solve that uses it brings its own scratch)."""
            h = self._handles.get(device)
            if h is None:
                h = _CoxHandle(self, device)
                self._handles[device] = h
            return h

        def _device_eval(self, eta, device=0, *, grad=True, hess=True, loss=True):
            """One evaluation of the family on the device (``adelie_hip_glm_cox_eval``): (grad, hess, loss), None where not
            asked for."""
            return self._device_handle(device).eval(eta, grad=grad, hess=hess, loss=loss)

    return _cox()


class _CoxHandle:
    """Owner of one ``adelie_hip_glm_cox`` handle."""

    def __init__(self, fam, device):
        b = _abi.hip_backend()
        self._b = b
        self.dtype = fam.dtype
        self.n = fam.status.shape[0]
        self.device = device
        h = _abi.C.c_void_p()
        start, stop, status, weights = [np.ascontiguousarray(a, dtype=fam.dtype)
                                        for a in (fam.start, fam.stop, fam.status, fam.weights)]
        strata = np.ascontiguousarray(fam.strata, dtype=np.int64)
        tie = _abi.TIE_EFRON if fam.tie_method == "efron" else _abi.TIE_BRESLOW
        b.check(b.fn("glm_cox_create")(int(device), _abi.dtype_code(fam.dtype), self.n, start.ctypes.data, stop.ctypes.data,
                                       status.ctypes.data, strata.ctypes.data, weights.ctypes.data, tie, _abi.C.byref(h)))
        self.h = h

    def eval(self, eta, *, grad=True, hess=True, loss=True):
        eta = np.ascontiguousarray(eta, dtype=self.dtype)
        if eta.shape != (self.n,):
            raise RuntimeError("eta must be (n,).")
        g = np.empty(self.n, dtype=self.dtype) if grad else None
        h = np.empty(self.n, dtype=self.dtype) if hess else None
        lo = _abi.C.c_double(0)
        self._b.check(self._b.fn("glm_cox_eval")(self.h, eta.ctypes.data, _abi.ptr(g), _abi.ptr(h),
                                                 _abi.C.byref(lo) if loss else None))
        return g, h, (lo.value if loss else None)

    def __del__(self):
        h = getattr(self, "h", None)
        if h is not None and h.value:
            try:
                self._b.fn("glm_cox_destroy")(h)
            except Exception:  # noqa: BLE001 (interpreter shutdown)
                pass
